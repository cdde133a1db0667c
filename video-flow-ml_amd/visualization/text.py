"""Text labels of the output video: the host path (numpy) and the compiler of the device plan (DESIGN.md section 9,
"Text").  The definition - the stroke font of visualization/stroke_font.py, positions in 1/64 px, capsule strokes, 16
samples per anti-aliased pixel, `out = (colour * n + dst * (16 - n) + 8) >> 4` - is integer only; tests/text_oracle.py
states it in full and is what this module and vfml_text_draw (vfml/csrc/text.hip) are held to, byte for byte.  It is the
project's own text and is not pinned against cv2.putText.

A frame's text is an ordered draw list; later operations blend over earlier ones, each inside its clip rectangle
(x0, y0, x1, y1), inclusive pixels:
    ("text", string, (x, y), S, thickness, (c0, c1, c2), aa, clip)      S = scale_of(font_scale); (x, y) as cv2's org
    ("dim", (x0, y0), (x1, y1), clip)                                    out = (3 * dst + 5) // 10, corners inclusive
Colours go to channels 0, 1, 2 in the picture's memory order.

`draw_ops` draws a list on the host.  `build_plan` compiles it once per job into the int32 plan vfml_text_draw reads
(include/vfml.h): operations whose pixel boxes overlap are merged into disjoint boxes, each with its operations in
order, so that one thread owns one pixel and no pixel is touched twice.
"""
import functools

import numpy as np

from .stroke_font import glyph

MARGIN = 5
MAX_SCALE, MAX_THICKNESS = 2048, 16           # font_scale <= 8: every product of the coverage test stays below 2^62
PLAN_MAGIC = 0x54584656                       # "VFXT"
PLAN_HEADER, BOX_WORDS, OP_WORDS, GLYPH_WORDS, SEG_WORDS = 8, 8, 12, 8, 4
OP_TEXT, OP_DIM = 0, 1
BLOCK_W, BLOCK_H = 32, 8                      # pixels of a box per thread block (vfml/csrc/text.hip)


def scale_of(font_scale):
    """S = round(font_scale * 256), halves up."""
    return int(np.floor(font_scale * 256 + 0.5))


def text_size(text, font_scale=0.4, thickness=1):
    """(width, height) of a string in pixels, in cv2.getTextSize's place."""
    S = scale_of(font_scale)
    A = sum(glyph(ch)[0] for ch in text)
    return ((A * S + 128) >> 8) + thickness, ((21 * S + 128) >> 8) + (thickness + 1) // 2


def anchor(position, text, font_scale, thickness, h, w):
    """Origin of a label in an h x w picture: one of the four named corners at margin 5 (reference
    video_composer.py:45-58; an unknown name is top-left), or the tuple itself."""
    if isinstance(position, tuple):
        return int(position[0]), int(position[1])
    tw, th = text_size(text, font_scale, thickness)
    if position == 'top-right':
        return w - tw - MARGIN, th + MARGIN
    if position == 'bottom-left':
        return MARGIN, h - MARGIN
    if position == 'bottom-right':
        return w - tw - MARGIN, h - MARGIN
    return MARGIN, th + MARGIN


# ---- draw lists of the layouts -------------------------------------------------------------------------------------------
def overlay_ops(text, position, h, w, tile=(0, 0), font_scale=0.4, color=(255, 255, 255), thickness=1):
    """add_text_overlay on an h x w picture at `tile` (x, y) of the frame (reference video_composer.py:60-63): black at
    thickness + 1, then `color` at thickness, anti-aliased, clipped to the picture."""
    x, y = anchor(position, text, font_scale, thickness, h, w)
    origin = (x + tile[0], y + tile[1])
    clip = (tile[0], tile[1], tile[0] + w - 1, tile[1] + h - 1)
    S = scale_of(font_scale)
    return [("text", text, origin, S, thickness + 1, (0, 0, 0), True, clip),
            ("text", text, origin, S, thickness, tuple(int(c) for c in color), True, clip)]


def side_by_side_ops(h, w, taa=0, model_name="VideoFlow", fast_mode=False, flow_format="gamedev"):
    """Labels of create_side_by_side (reference video_composer.py:86-116), tiles of h x w, in frame coordinates.
    taa: 0 original | flow, 1 the 3-wide frame with one TAA tile, 2 the 2x2 grid."""
    mode = " (Fast)" if fast_mode else ""
    ops = overlay_ops(f"Original{mode}", 'top-left', h, w)
    ops += overlay_ops(f"Optical Flow{mode}", 'top-left', h, w, (w, 0))
    ops += overlay_ops(f"{model_name} ({flow_format.upper()})", 'bottom-left', h, w, (w, 0))
    if taa:
        tile = (0, h) if taa == 2 else (2 * w, 0)
        ops += overlay_ops("TAA + Inv.Flow", 'top-left', h, w, tile)
        ops += overlay_ops("Alpha: 0.1", 'bottom-left', h, w, tile)
    if taa == 2:
        ops += overlay_ops("TAA Simple", 'top-left', h, w, (w, h))
        ops += overlay_ops("Alpha: 0.1", 'bottom-left', h, w, (w, h))
    return ops


GRID6_LABELS = ("Original", "External Flow", "TAA + Original Flow", "TAA Simple", "TAA + External Flow",
                "Flow Difference")


def grid6_ops(h, w):
    """The six labels of create_6_video_grid (reference flow_processor.py:1261-1267): drawn on the whole 3h x 2w frame
    at (10, 10) of each tile, as the reference draws them after the tiles are joined."""
    ops = []
    for k, text in enumerate(GRID6_LABELS):
        ops += overlay_ops(text, ((k % 2) * w + 10, (k // 2) * h + 10), 3 * h, 2 * w)
    return ops


def legend_ops(h, w, tile=(0, 0), levels=(0.1, 0.5, 1.0, 2.0)):
    """The numbers beside the difference legend's squares (reference flow_processor.py:560-576) on an h x w overlay at
    `tile`: scale 0.3, thickness 1, not anti-aliased, a black shadow at (+1, +1) under white."""
    ops = []
    clip = (tile[0], tile[1], tile[0] + w - 1, tile[1] + h - 1)
    S = scale_of(0.3)
    for i in range(len(levels) + 1):
        label = f"{levels[i]:.3f}" if i < len(levels) else f">{levels[i - 1]:.3f}"
        x, y = 10 + 45 * i + 12 + 3 + tile[0], h - 20 - 4 + tile[1]
        ops.append(("text", label, (x + 1, y + 1), S, 1, (0, 0, 0), False, clip))
        ops.append(("text", label, (x, y), S, 1, (255, 255, 255), False, clip))
    return ops


def video_grid_label_ops(label, h, w):
    """create_video_grid's label on an h x w cell (reference video_composer.py:192-218): the dimmed backdrop, then each
    line at scale 0.7, thickness 2 over a black outline of thickness 4."""
    lines = label.split('\n')
    width = max(text_size(line, 0.7, 2)[0] for line in lines)
    clip = (0, 0, w - 1, h - 1)
    ops = [("dim", (0, 0), (width + 15, len(lines) * 30 + 10), clip)]
    S = scale_of(0.7)
    for k, line in enumerate(lines):
        ops.append(("text", line, (8, 25 + 30 * k), S, 4, (0, 0, 0), True, clip))
        ops.append(("text", line, (8, 25 + 30 * k), S, 2, (255, 255, 255), True, clip))
    return ops


# ---- geometry shared by the host path and the plan -------------------------------------------------------------------------
def _check_text(S, thickness):
    if not 1 <= S <= MAX_SCALE:
        raise ValueError(f"text: font scale {S / 256:g} outside (0, {MAX_SCALE // 256}]")
    if not 1 <= thickness <= MAX_THICKNESS:
        raise ValueError(f"text: thickness {thickness} outside 1..{MAX_THICKNESS}")


def _string_glyphs(text, S):
    """Per character with segments: int64 [K, 4] (X0, Y0, X1, Y1) in 1/64 px relative to the string's origin."""
    out, pen = [], 0
    for ch in text:
        adv, segs = glyph(ch)
        if segs:
            g = np.array(segs, np.int64)
            rel = np.empty_like(g)
            rel[:, 0::2] = ((pen + g[:, 0::2]) * S + 2) >> 2
            rel[:, 1::2] = -((g[:, 1::2] * S + 2) >> 2)
            out.append(rel)
        pen += adv
    return out


def _clip_to(clip, h, w):
    return max(int(clip[0]), 0), max(int(clip[1]), 0), min(int(clip[2]), w - 1), min(int(clip[3]), h - 1)


def _dim_rect(op, h, w):
    _, c0, c1, clip = op
    cx0, cy0, cx1, cy1 = _clip_to(clip, h, w)
    return (max(min(c0[0], c1[0]), cx0), max(min(c0[1], c1[1]), cy0), min(max(c0[0], c1[0]), cx1),
            min(max(c0[1], c1[1]), cy1))


# ---- host path -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=512)
def _text_coverage(h, w, op):
    """-> (x0, y0, n): n int64 [rows, cols] samples inside the string for the pixel block at (x0, y0); None if empty.
    Kept per operation: a job's labels are the same on every frame, so only the blend is per-frame work."""
    _, text, origin, S, thickness, _, aa, clip = op
    _check_text(S, thickness)
    r = 32 * thickness
    ox, oy = 64 * int(origin[0]), 64 * int(origin[1])
    glyphs = _string_glyphs(text, S)
    if not glyphs:
        return None
    allseg = np.concatenate(glyphs)
    cx0, cy0, cx1, cy1 = _clip_to(clip, h, w)
    x0 = max(cx0, (ox + int(allseg[:, 0::2].min()) - r) >> 6)
    x1 = min(cx1, (ox + int(allseg[:, 0::2].max()) + r) >> 6)
    y0 = max(cy0, (oy + int(allseg[:, 1::2].min()) - r) >> 6)
    y1 = min(cy1, (oy + int(allseg[:, 1::2].max()) + r) >> 6)
    if x0 > x1 or y0 > y1:
        return None
    sub = np.array([4, 12, 20, 28] if aa else [32], np.int64)                  # 4 (2 i + 1), or the pixel centre
    hit = np.zeros((len(sub), len(sub), y1 - y0 + 1, x1 - x0 + 1), bool)       # [j, i, y, x]
    for seg in glyphs:
        gx0 = max(x0, (ox + int(seg[:, 0::2].min()) - r) >> 6)
        gx1 = min(x1, (ox + int(seg[:, 0::2].max()) + r) >> 6)
        gy0 = max(y0, (oy + int(seg[:, 1::2].min()) - r) >> 6)
        gy1 = min(y1, (oy + int(seg[:, 1::2].max()) + r) >> 6)
        if gx0 > gx1 or gy0 > gy1:
            continue
        # samples [1, j, i, y, x] against segments [K, 1, 1, 1, 1]
        px = (64 * np.arange(gx0, gx1 + 1, dtype=np.int64)[None, None, None, None, :] - ox
              + sub[None, None, :, None, None])
        py = (64 * np.arange(gy0, gy1 + 1, dtype=np.int64)[None, None, None, :, None] - oy
              + sub[None, :, None, None, None])
        ax, ay, bx, by = (seg[:, k][:, None, None, None, None] for k in range(4))
        dx, dy = bx - ax, by - ay
        L2 = dx * dx + dy * dy
        qx, qy = px - ax, py - ay
        u = qx * dx + qy * dy
        c = qx * dy - qy * dx
        r2 = r * r
        inside = np.where(u <= 0, qx * qx + qy * qy <= r2,
                          np.where(u >= L2, (px - bx) ** 2 + (py - by) ** 2 <= r2, c * c <= r2 * L2))
        hit[:, :, gy0 - y0:gy1 - y0 + 1, gx0 - x0:gx1 - x0 + 1] |= inside.any(0)
    n = hit.sum((0, 1), dtype=np.int64) * (1 if aa else 16)
    n.setflags(write=False)
    return x0, y0, n


def draw_ops(img, ops):
    """Draw a list of operations on a uint8 [h, w, 3] picture; returns a new picture (the host path)."""
    out = np.array(img, dtype=np.uint8)
    h, w = out.shape[:2]
    for op in ops:
        if op[0] == "text":
            got = _text_coverage(h, w, (*op[:2], (int(op[2][0]), int(op[2][1])), int(op[3]), int(op[4]),
                                        tuple(int(c) for c in op[5]), bool(op[6]), tuple(int(v) for v in op[7])))
            if got is None:
                continue
            x0, y0, n = got
            dst = out[y0:y0 + n.shape[0], x0:x0 + n.shape[1]].astype(np.int64)
            colour = np.array(op[5], np.int64)[None, None, :]
            out[y0:y0 + n.shape[0], x0:x0 + n.shape[1]] = (colour * n[:, :, None] + dst * (16 - n[:, :, None]) + 8) >> 4
        elif op[0] == "dim":
            xa, ya, xb, yb = _dim_rect(op, h, w)
            if xa <= xb and ya <= yb:
                out[ya:yb + 1, xa:xb + 1] = (3 * out[ya:yb + 1, xa:xb + 1].astype(np.int64) + 5) // 10
        else:
            raise ValueError(f"text: unknown operation {op[0]!r}")
    return out


def draw_text(frame, text, position='top-left', font_scale=0.4, color=(255, 255, 255), thickness=1):
    """A label with its outline on a picture (the two operations of add_text_overlay); returns a new picture."""
    h, w = frame.shape[:2]
    return draw_ops(frame, overlay_ops(text, position, h, w, font_scale=font_scale, color=color, thickness=thickness))


# ---- device plan -----------------------------------------------------------------------------------------------------------
def _intersects(a, b):
    return a[0] <= b[2] and b[0] <= a[2] and a[1] <= b[3] and b[1] <= a[3]


def build_plan(ops, frame_h, frame_w):
    """Compile a draw list for a frame_h x frame_w frame into the int32 plan of vfml_text_draw (layout: include/vfml.h).
    Operations that cannot touch the frame are dropped; the rest are grouped into disjoint pixel boxes - operations
    whose boxes overlap share one, merged until no two boxes intersect - each with its operations in list order.
    Words 2..3 (the address of the plan's device copy) are left 0: vfml.hip.TextPlan fills them."""
    h, w = int(frame_h), int(frame_w)
    strings, glyph_rows, seg_rows = {}, [], []
    kept = []                                   # (pixel box, op words without the glyph range, string key)
    for op in ops:
        if op[0] == "dim":
            box = _dim_rect(op, h, w)
            if box[0] > box[2] or box[1] > box[3]:
                continue
            kept.append((box, [OP_DIM, *box, 0, 0, 0, 0, 0], None))
            continue
        if op[0] != "text":
            raise ValueError(f"text: unknown operation {op[0]!r}")
        _, text, origin, S, thickness, colour, aa, clip = op
        _check_text(S, thickness)
        key = (text, S)
        if key not in strings:
            first = len(glyph_rows)
            for rel in _string_glyphs(text, S):
                glyph_rows.append([int(rel[:, 0::2].min()), int(rel[:, 1::2].min()), int(rel[:, 0::2].max()),
                                   int(rel[:, 1::2].max()), len(seg_rows), len(rel), 0, 0])
                seg_rows += rel.tolist()
            strings[key] = (first, len(glyph_rows) - first)
        first, count = strings[key]
        if count == 0:
            continue
        r = 32 * thickness
        ox, oy = 64 * int(origin[0]), 64 * int(origin[1])
        g = np.array(glyph_rows[first:first + count])
        cx0, cy0, cx1, cy1 = _clip_to(clip, h, w)
        box = (max(cx0, (ox + int(g[:, 0].min()) - r) >> 6), max(cy0, (oy + int(g[:, 1].min()) - r) >> 6),
               min(cx1, (ox + int(g[:, 2].max()) + r) >> 6), min(cy1, (oy + int(g[:, 3].max()) + r) >> 6))
        if box[0] > box[2] or box[1] > box[3]:
            continue
        packed = int(colour[0]) | int(colour[1]) << 8 | int(colour[2]) << 16
        kept.append((box, [OP_TEXT, cx0, cy0, cx1, cy1, packed, r, int(bool(aa)), ox, oy], key))
    # merge overlapping boxes (their bounding rectangle) until all are disjoint
    groups = [[list(box), [k]] for k, (box, _, _) in enumerate(kept)]
    merged = True
    while merged:
        merged = False
        for a in range(len(groups)):
            for b in range(a + 1, len(groups)):
                if _intersects(groups[a][0], groups[b][0]):
                    ba, bb = groups[a][0], groups[b][0]
                    groups[a] = [[min(ba[0], bb[0]), min(ba[1], bb[1]), max(ba[2], bb[2]), max(ba[3], bb[3])],
                                 sorted(groups[a][1] + groups[b][1])]
                    del groups[b]
                    merged = True
                    break
            if merged:
                break
    box_rows, op_rows, blocks = [], [], 0
    for box, members in groups:
        nblocks = -(-(box[2] - box[0] + 1) // BLOCK_W) * -(-(box[3] - box[1] + 1) // BLOCK_H)
        box_rows.append([*box, len(op_rows), len(members), blocks, 0])
        blocks += nblocks
        for k in members:
            _, words, key = kept[k]
            op_rows.append(words + list(strings[key] if key is not None else (0, 0)))
    total = PLAN_HEADER + BOX_WORDS * len(box_rows) + OP_WORDS * len(op_rows) + GLYPH_WORDS * len(glyph_rows) + \
        SEG_WORDS * len(seg_rows)
    plan = [PLAN_MAGIC, total, 0, 0, len(box_rows), len(op_rows), len(glyph_rows), len(seg_rows)]
    for rows in (box_rows, op_rows, glyph_rows, seg_rows):
        for row in rows:
            plan += row
    assert len(plan) == total
    return np.array(plan, dtype=np.int32)


def plan_boxes(plan):
    """[(x0, y0, x1, y1, first operation, operations), ...] of a plan."""
    n = int(plan[4])
    rows = np.asarray(plan[PLAN_HEADER:PLAN_HEADER + BOX_WORDS * n]).reshape(n, BOX_WORDS)
    return [tuple(int(v) for v in row[:6]) for row in rows]
