"""The project's text, as defined in DESIGN.md section 9 ("Text"), in plain numpy: the oracle of visualization/text.py
(the host path) and of vfml_text_draw (the kernel).  Slow on purpose: every segment is tested on its own, sample by
sample, with the rule as it is written down.  Integer only.

Units: 1/64 px.  S = round(font_scale * 256).  A string at origin (x, y) - the left end of its baseline, in pixels, as
cv2.putText's `org` - puts glyph vertex (gx, gy) at pen offset P (font units) at
    X = 64 x + (((P + gx) * S + 2) >> 2)        Y = 64 y - ((gy * S + 2) >> 2).
A stroke of thickness t covers the points within r = 32 t of a segment a -> b.  With d = b - a, L2 = d.d, q = p - a,
u = q.d and c = q x d, sample p is inside when
    u <= 0   and |p - a|^2 <= r^2,   or   u >= L2 and |p - b|^2 <= r^2,   or   0 < u < L2 and c^2 <= r^2 L2.
Widest intermediate: c^2.  A segment is only tested on the pixels of its bounding box grown by r + 64 units, where
|q| < 2^15 and |d| < 2^14 (font_scale <= 8, thickness <= 16), so |c| < 2^30 and c^2 < 2^60: int64 everywhere.
Anti-aliased: 16 samples per pixel at (64 px + 4 (2 i + 1), 64 py + 4 (2 j + 1)), i, j = 0..3, n = samples inside any
segment of the string; otherwise one sample at (64 px + 32, 64 py + 32) and n = 0 or 16.
    out = (colour * n + dst * (16 - n) + 8) >> 4          per channel, channels 0, 1, 2 in memory order.

Operations, drawn in list order, each clipped to its `clip` = (x0, y0, x1, y1), inclusive pixels:
    ("text", string, (x, y), S, thickness, (c0, c1, c2), aa, clip)
    ("dim", (x0, y0), (x1, y1), clip)          out = (3 * dst + 5) // 10 inside the rectangle, corners inclusive
"""
import numpy as np

from visualization.stroke_font import GLYPHS

MARGIN = 5
LEGEND_LEVELS = (0.1, 0.5, 1.0, 2.0)


def scale_of(font_scale):
    return int(np.floor(font_scale * 256 + 0.5))


def glyph_of(ch):
    return GLYPHS[ch] if ch in GLYPHS else GLYPHS['?']


def text_size(text, font_scale, thickness):
    S = scale_of(font_scale)
    A = sum(glyph_of(ch)[0] for ch in text)
    return ((A * S + 128) >> 8) + thickness, ((21 * S + 128) >> 8) + (thickness + 1) // 2


def anchor(position, text, font_scale, thickness, h, w):
    """The origin of a label in an h x w picture (reference video_composer.py:45-58)."""
    if isinstance(position, tuple):
        return position
    tw, th = text_size(text, font_scale, thickness)
    if position == 'top-right':
        return (w - tw - MARGIN, th + MARGIN)
    if position == 'bottom-left':
        return (MARGIN, h - MARGIN)
    if position == 'bottom-right':
        return (w - tw - MARGIN, h - MARGIN)
    return (MARGIN, th + MARGIN)


def string_segments(text, origin, S):
    """Every segment of a string in 1/64 px: [(X0, Y0, X1, Y1), ...]."""
    out, pen = [], 0
    for ch in text:
        adv, segs = glyph_of(ch)
        for gx0, gy0, gx1, gy1 in segs:
            out.append((64 * origin[0] + (((pen + gx0) * S + 2) >> 2), 64 * origin[1] - ((gy0 * S + 2) >> 2),
                        64 * origin[0] + (((pen + gx1) * S + 2) >> 2), 64 * origin[1] - ((gy1 * S + 2) >> 2)))
        pen += adv
    return out


def _inside(px, py, seg, r):
    """Samples (px, py), int64 arrays in units -> bool array: within r of the segment."""
    ax, ay, bx, by = seg
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    qx, qy = px - ax, py - ay
    u = qx * dx + qy * dy
    c = qx * dy - qy * dx
    r2 = r * r
    near_a = (u <= 0) & (qx * qx + qy * qy <= r2)
    near_b = (u >= L2) & ((px - bx) ** 2 + (py - by) ** 2 <= r2)
    between = (u > 0) & (u < L2) & (c * c <= r2 * L2)
    return near_a | near_b | between


def coverage(h, w, text, origin, S, thickness, aa, clip):
    """n (0..16) per pixel of an h x w picture."""
    r = 32 * thickness
    offsets = [(4 * (2 * i + 1), 4 * (2 * j + 1)) for j in range(4) for i in range(4)] if aa else [(32, 32)]
    hit = np.zeros((len(offsets), h, w), bool)
    cx0, cy0, cx1, cy1 = max(clip[0], 0), max(clip[1], 0), min(clip[2], w - 1), min(clip[3], h - 1)
    for seg in string_segments(text, origin, S):
        x0 = max(cx0, (min(seg[0], seg[2]) - r - 64) >> 6)
        x1 = min(cx1, (max(seg[0], seg[2]) + r + 64) >> 6)
        y0 = max(cy0, (min(seg[1], seg[3]) - r - 64) >> 6)
        y1 = min(cy1, (max(seg[1], seg[3]) + r + 64) >> 6)
        if x0 > x1 or y0 > y1:
            continue
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
        for k, (ox, oy) in enumerate(offsets):
            hit[k, y0:y1 + 1, x0:x1 + 1] |= _inside(64 * xx + ox, 64 * yy + oy, seg, r)
    n = hit.sum(0)
    return n if aa else 16 * n


def draw_ops(img, ops):
    """Draw a list of operations into a uint8 [h, w, 3] picture; returns a new picture."""
    out = np.array(img, dtype=np.int64)
    h, w = out.shape[:2]
    for op in ops:
        if op[0] == "text":
            _, text, origin, S, thickness, colour, aa, clip = op
            n = coverage(h, w, text, origin, S, thickness, aa, clip)[:, :, None]
            out = (np.array(colour, np.int64)[None, None, :] * n + out * (16 - n) + 8) >> 4
        elif op[0] == "dim":
            _, c0, c1, clip = op
            xa, xb = sorted((c0[0], c1[0]))
            ya, yb = sorted((c0[1], c1[1]))
            xa, ya = max(xa, clip[0], 0), max(ya, clip[1], 0)
            xb, yb = min(xb, clip[2], w - 1), min(yb, clip[3], h - 1)
            if xa <= xb and ya <= yb:
                out[ya:yb + 1, xa:xb + 1] = (3 * out[ya:yb + 1, xa:xb + 1] + 5) // 10
        else:
            raise ValueError(op[0])
    return out.astype(np.uint8)


# ---- the label lists of each layout ------------------------------------------------------------------------------------
def overlay_ops(text, position, h, w, tile=(0, 0), font_scale=0.4, colour=(255, 255, 255), thickness=1, clip=None):
    """add_text_overlay on an h x w picture whose top-left corner is at `tile` (x, y) of the frame: black at
    thickness + 1, then `colour` at thickness, both anti-aliased, clipped to the picture."""
    x, y = anchor(position, text, font_scale, thickness, h, w)
    origin = (x + tile[0], y + tile[1])
    clip = clip or (tile[0], tile[1], tile[0] + w - 1, tile[1] + h - 1)
    S = scale_of(font_scale)
    return [("text", text, origin, S, thickness + 1, (0, 0, 0), True, clip),
            ("text", text, origin, S, thickness, tuple(colour), True, clip)]


def side_by_side_ops(h, w, taa=0, model_name="VideoFlow", fast_mode=False, flow_format="gamedev"):
    """Labels of create_side_by_side (reference video_composer.py:86-116) for tiles of h x w; taa: 0 side by side, 1 the
    3-wide single-TAA frame, 2 the 2x2 grid."""
    mode = " (Fast)" if fast_mode else ""
    ops = overlay_ops(f"Original{mode}", 'top-left', h, w)
    ops += overlay_ops(f"Optical Flow{mode}", 'top-left', h, w, (w, 0))
    ops += overlay_ops(f"{model_name} ({flow_format.upper()})", 'bottom-left', h, w, (w, 0))
    if taa:
        t = (0, h) if taa == 2 else (2 * w, 0)
        ops += overlay_ops("TAA + Inv.Flow", 'top-left', h, w, t)
        ops += overlay_ops("Alpha: 0.1", 'bottom-left', h, w, t)
    if taa == 2:
        ops += overlay_ops("TAA Simple", 'top-left', h, w, (w, h))
        ops += overlay_ops("Alpha: 0.1", 'bottom-left', h, w, (w, h))
    return ops


def legend_ops(h, w, tile=(0, 0)):
    """The numbers of the difference legend (reference flow_processor.py:560-576) on an h x w overlay at `tile`."""
    ops = []
    clip = (tile[0], tile[1], tile[0] + w - 1, tile[1] + h - 1)
    S = scale_of(0.3)
    for i in range(5):
        label = f"{LEGEND_LEVELS[i]:.3f}" if i < 4 else ">" + f"{2.0:.3f}"
        tx, ty = 10 + 45 * i + 12 + 3 + tile[0], h - 20 - 4 + tile[1]
        ops.append(("text", label, (tx + 1, ty + 1), S, 1, (0, 0, 0), False, clip))
        ops.append(("text", label, (tx, ty), S, 1, (255, 255, 255), False, clip))
    return ops


def grid6_ops(h, w):
    """The six labels of create_6_video_grid (reference flow_processor.py:1261-1267), drawn on the whole 3h x 2w frame."""
    ops = []
    for text, origin in (("Original", (10, 10)), ("External Flow", (w + 10, 10)), ("TAA + Original Flow", (10, h + 10)),
                         ("TAA Simple", (w + 10, h + 10)), ("TAA + External Flow", (10, 2 * h + 10)),
                         ("Flow Difference", (w + 10, 2 * h + 10))):
        ops += overlay_ops(text, origin, 3 * h, 2 * w)
    return ops


def video_grid_label_ops(label, h, w):
    """create_video_grid's label on one h x w cell: the backdrop, then every line at scale 0.7, thickness 2 with a
    black outline of thickness 4."""
    lines = label.split('\n')
    width = max(text_size(line, 0.7, 2)[0] for line in lines)
    clip = (0, 0, w - 1, h - 1)
    ops = [("dim", (0, 0), (width + 15, len(lines) * 30 + 10), clip)]
    S = scale_of(0.7)
    for k, line in enumerate(lines):
        ops.append(("text", line, (8, 25 + 30 * k), S, 4, (0, 0, 0), True, clip))
        ops.append(("text", line, (8, 25 + 30 * k), S, 2, (255, 255, 255), True, clip))
    return ops
