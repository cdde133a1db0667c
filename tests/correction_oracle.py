"""ORACLE (test infrastructure, never imported by the product): a numpy restatement of the batch flow-cache correction
(the reference's correction_worker.py worker, :221-341) and of the three OpenCV primitives it calls, as this project
defines them.  The definitions of cvtColor / phaseCorrelate / matchTemplate are written from the
OpenCV 4.x algorithms and are not pinned against cv2 itself (it is not a dependency of this project).

Scalar types follow numpy >= 2 promotion (NEP 50) step by step, because the worker mixes numpy scalars and Python
floats: a float32 flow value divided or shifted by a Python float stays float32; int64 pixel coordinates minus a
float32 value promote to float64.  tests/golden/correction.npz (cut from the reference's own worker with these
primitives) pins it; tests/test_correction_cpu.py holds it to those bytes."""
import math

import numpy as np

F32 = np.float32
RGB_MAX = math.sqrt(195075.0)          # sqrt(3 * 255^2)
EPS52 = 2.0 ** -52

DEFAULT_CONSTANTS = {"GOOD_QUALITY_THRESHOLD": 0.8, "FINE_CORRECTION_THRESHOLD": 0.9, "DETAIL_ANALYSIS_REGION_SIZE": 25,
                     "TEMPLATE_RADIUS": 5.5, "SEARCH_RADIUS": 25}


# ---- primitives ---------------------------------------------------------------------------------------------------
def grey(img):
    """RGB u8 -> grey u8 in exact integers (cvtColor RGB2GRAY)."""
    v = img.astype(np.int64)
    return ((v[..., 0] * 4899 + v[..., 1] * 9617 + v[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def similarity(a, b):
    """Colour similarity of two u8 RGB triples (reference calculate_pixel_quality), float64."""
    a = [float(v) for v in a]
    b = [float(v) for v in b]
    d = [a[i] - b[i] for i in range(3)]
    rgb = 1.0 - math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / RGB_MAX
    mad = 1.0 - ((abs(d[0]) + abs(d[1])) + abs(d[2])) / 3.0 / 255.0
    na = math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    nb = math.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
    if na > 1e-6 and nb > 1e-6:
        cs = (((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) / (na * nb) + 1.0) / 2.0
    else:
        cs = 1.0 - abs(na - nb) / RGB_MAX
    return (rgb + mad + cs) / 3.0


def _slice_len(start, stop, n):
    """len(range(n)[start:stop]) for start >= 0 (Python slice rules: a negative stop counts from the end)."""
    if stop < 0:
        stop = max(0, n + stop)
    start, stop = min(start, n), min(stop, n)
    return start, max(0, stop - start)


def extract_region(img, cx, cy, radius):
    """(region, (x1, y1)): the slice [y1:y2, x1:x2] around (cx, cy), zero-padded at the bottom/right up to 2r."""
    h, w = img.shape[:2]
    x1, y1 = max(0, int(cx - radius)), max(0, int(cy - radius))
    x2, y2 = min(w, int(cx + radius)), min(h, int(cy + radius))
    sx, nx = _slice_len(x1, x2, w)
    sy, ny = _slice_len(y1, y2, h)
    side = int(2 * radius)
    out = np.zeros((max(ny, side), max(nx, side)) + img.shape[2:], img.dtype)
    out[:ny, :nx] = img[sy:sy + ny, sx:sx + nx]
    return out, (x1, y1)


def twiddles(n):
    """[2, n] float64: cos and sin of 2 pi m / n (the table the kernel is handed)."""
    ang = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.stack([np.cos(ang), np.sin(ang)])


def _dft_pass(re, im, tw, axis, inverse):
    """Direct length-N DFT along axis (-1 rows, -2 columns), terms summed in ascending input index."""
    n = re.shape[axis]
    c = tw[0]
    s = tw[1] if inverse else -tw[1]
    k = np.arange(n)
    acc_re = np.zeros_like(re)
    acc_im = np.zeros_like(im)
    for j in range(n):
        m = (j * k) % n
        wc, ws = c[m], s[m]
        if axis == -1:
            a, b = re[..., :, j:j + 1], im[..., :, j:j + 1]
        else:
            a, b = re[..., j:j + 1, :], im[..., j:j + 1, :]
            wc, ws = wc[:, None], ws[:, None]
        acc_re = acc_re + (a * wc - b * ws)
        acc_im = acc_im + (a * ws + b * wc)
    return acc_re, acc_im


def dft2(re, im, tw, inverse=False):
    re, im = _dft_pass(re, im, tw, -1, inverse)
    return _dft_pass(re, im, tw, -2, inverse)


def phase_correlate(a, b):
    """(dx, dy) of two equal-size float images (phaseCorrelate without a window); sizes whose optimal DFT size is
    themselves (50 for the default geometry)."""
    m, n = a.shape[-2:]
    assert m == n, "square regions only"
    tw = twiddles(n)
    zero = np.zeros(a.shape, np.float64)
    ar, ai = dft2(a.astype(np.float64), zero, tw)
    br, bi = dft2(b.astype(np.float64), zero, tw)
    nbi = -bi
    pr = ar * br - ai * nbi
    pi = ar * nbi + ai * br
    mag = np.sqrt(pr * pr + pi * pi)
    den = mag * mag + EPS52
    cr, ci = pr * mag / den, pi * mag / den
    rr, _ = dft2(cr, ci, tw, inverse=True)
    r = np.roll(rr, (m // 2, n // 2), axis=(-2, -1))           # fftShift (even sizes)
    flat = int(np.argmax(r))
    py, px = divmod(flat, n)
    cx = cy = s = 0.0
    for y in range(max(0, py - 2), min(m - 1, py + 2) + 1):
        for x in range(max(0, px - 2), min(n - 1, px + 2) + 1):
            v = float(r[y, x])
            cx += x * v
            cy += y * v
            s += v
    s += EPS52
    return n / 2.0 - cx / s, m / 2.0 - cy / s


def match_template(search, templ):
    """TM_CCOEFF_NORMED of a 3-channel u8 template over a u8 search area -> float32 [R-th+1, C-tw+1]."""
    th, tw_ = templ.shape[:2]
    n = th * tw_
    S = search.astype(np.int64)
    T = templ.astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(S, (th, tw_), axis=(0, 1))     # [oy, ox, 3, th, tw]
    Tt = T.transpose(2, 0, 1)
    sti = np.einsum("yxcij,cij->yxc", win, Tt)
    si = win.sum(axis=(3, 4))
    si2 = (win * win).sum(axis=(3, 4))
    st = Tt.sum(axis=(1, 2))
    st2 = (Tt * Tt).sum(axis=(1, 2))
    num = (n * sti - st * si).sum(-1)
    tv = int((n * st2 - st * st).sum())
    wv = (n * si2 - si * si).sum(-1)
    if tv == 0:
        return np.ones(num.shape, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = num.astype(np.float64) / (math.sqrt(float(tv)) * np.sqrt(wv.astype(np.float64)))
    r = np.where(wv == 0, 0.0, np.minimum(np.maximum(r, -1.0), 1.0))
    return r.astype(F32)


def spiral(width, height):
    """Offsets outwards from the centre in the worker's spiral order."""
    x = y = 0
    dx, dy = 0, -1
    out = []
    for _ in range(max(width, height) ** 2):
        if -width / 2 < x <= width / 2 and -height / 2 < y <= height / 2:
            out.append((x, y))
        if x == y or (x < 0 and x == -y) or (x > 0 and x == 1 - y):
            dx, dy = -dy, dx
        x, y = x + dx, y + dy
    return out


# ---- the worker's steps ------------------------------------------------------------------------------------------
def coarse(frame1, frame2, x, y, lod_vec, r):
    """-> (shift, flow (float32 pair), target (float64 pair), similarity)."""
    lx, ly = lod_vec
    r1, _ = extract_region(frame1, x, y, r)
    r2, _ = extract_region(frame2, float(x) - float(lx), float(y) - float(ly), r)
    g1, g2 = grey(r1), grey(r2)
    mh, mw = min(g1.shape[0], g2.shape[0]), min(g1.shape[1], g2.shape[1])
    if mh < 2 or mw < 2:
        dx = dy = 0.0
    else:
        dx, dy = phase_correlate(g1[:mh, :mw], g2[:mh, :mw])
    fx, fy = F32(lx - F32(dx)), F32(ly - F32(dy))
    tx, ty = float(x) - float(fx), float(y) - float(fy)
    h, w = frame1.shape[:2]
    sim = 0.0
    if 0 <= tx < w and 0 <= ty < h:
        sim = similarity(frame1[y, x], frame2[int(ty), int(tx)])
    return (dx, dy), (fx, fy), (tx, ty), sim


def fine(frame1, frame2, x, y, target, trad, srad, good):
    """-> None or (flow (float64 pair), similarity)."""
    templ, _ = extract_region(frame1, x, y, trad)
    area, (sx1, sy1) = extract_region(frame2, target[0], target[1], srad)
    if templ.shape[0] != int(2 * trad) or area.shape[0] != int(2 * srad):
        return None
    res = match_template(area, templ)
    ly, lx = divmod(int(np.argmax(res)), res.shape[1])
    pcx, pcy = sx1 + lx + trad, sy1 + ly + trad
    h, w = frame2.shape[:2]
    if not (0 <= pcx < w and 0 <= pcy < h):
        return None
    src = frame1[y, x]
    best, sim = (pcx, pcy), similarity(src, frame2[int(pcy), int(pcx)])
    if not sim > good:
        side = int(trad * 2)
        for dx, dy in spiral(side, side):
            cx, cy = pcx + dx, pcy + dy
            if 0 <= cx < w and 0 <= cy < h:
                s = similarity(src, frame2[int(cy), int(cx)])
                if s > good:
                    best, sim = (cx, cy), s
                    break
    return (float(x) - best[0], float(y) - best[1]), sim


RECORD_FIELDS = ("pixel", "orig_sim", "lod_x", "lod_y", "shift_x", "shift_y", "coarse_x", "coarse_y", "coarse_sim",
                 "fine_attempted", "fine_valid", "fine_x", "fine_y", "fine_sim", "accepted", "reserved")


def correct_pixel(frame1, frame2, flow, lod, x, y, c):
    """One bad pixel -> (record (float64[16]), new vector or None).  flow: float32 at frame resolution."""
    h, w = frame1.shape[:2]
    lh, lw = lod.shape[:2]
    rec = np.zeros(16, np.float64)
    rec[0] = y * w + x
    fx, fy = flow[y, x, 0], flow[y, x, 1]
    ox, oy = int(round(float(x) - float(fx))), int(round(float(y) - float(fy)))
    orig = similarity(frame1[y, x], frame2[oy, ox]) if (0 <= ox < w and 0 <= oy < h) else 0.0
    sx, sy = lw / w, lh / h
    tx, ty = max(0, min(int(x * sx), lw - 1)), max(0, min(int(y * sy), lh - 1))
    lvx, lvy = F32(lod[ty, tx, 0] / F32(sx)), F32(lod[ty, tx, 1] / F32(sy))
    shift, cflow, ctarget, csim = coarse(frame1, frame2, x, y, (lvx, lvy), c["DETAIL_ANALYSIS_REGION_SIZE"])
    rec[1:9] = [orig, lvx, lvy, shift[0], shift[1], cflow[0], cflow[1], csim]
    final, fsim = (float(cflow[0]), float(cflow[1])), csim
    good = c["GOOD_QUALITY_THRESHOLD"]
    if csim < c["FINE_CORRECTION_THRESHOLD"]:
        rec[9] = 1
        fr = fine(frame1, frame2, x, y, ctarget, c["TEMPLATE_RADIUS"], c["SEARCH_RADIUS"], good)
        if fr is not None:
            rec[10:14] = [1, fr[0][0], fr[0][1], fr[1]]
            if fr[1] > csim:
                final, fsim = fr
    if fsim > good or fsim > orig:
        rec[14] = 1
        return rec, (F32(final[0]), F32(final[1]))
    return rec, None


def bad_pixels(frame1, frame2, flow, good):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.quality_map import quality_map
    return quality_map(frame1, frame2, flow, good)[..., 0] > 0


def correct_frame(frame1, frame2, flow, lod, constants=None, pixels=None):
    """-> (corrected flow, initial bad count, final bad count, records [n, 16]).  `pixels`: raster indices of a
    subset of the bad pixels to evaluate (records only; the flow and the final count then cover that subset)."""
    c = dict(DEFAULT_CONSTANTS if constants is None else constants)
    good = c["GOOD_QUALITY_THRESHOLD"]
    bad = bad_pixels(frame1, frame2, flow, good)
    ys, xs = np.nonzero(bad)
    h, w = frame1.shape[:2]
    if pixels is not None:
        keep = np.isin(ys * w + xs, pixels)
        ys, xs = ys[keep], xs[keep]
    out = flow.copy()
    recs = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        rec, vec = correct_pixel(frame1, frame2, flow, lod, x, y, c)
        recs.append(rec)
        if vec is not None:
            out[y, x] = vec
    final = int(bad_pixels(frame1, frame2, out, good).sum())
    return out, int(bad.sum()), final, np.array(recs, np.float64).reshape(-1, 16)


# ---- fixture scenes (tests/golden/correction.npz) ------------------------------------------------------------------
def fixture_scenes(gold):
    """[(tag, scene)] with scene = dict(frames, flows {i: flow}, lods {(i, level): lod}, indices, ext, written,
    counts [[frame, initial, final]], records, corrected {i: flow}, corrected_bytes {i: bytes of a .flo})."""
    out = []
    for tag in ("a", "b"):
        sc = {"frames": list(gold[f"{tag}_frames"]), "flows": {}, "lods": {}, "corrected": {}, "corrected_bytes": {},
              "indices": [int(v) for v in gold[f"{tag}_indices"]], "ext": str(gold[f"{tag}_ext"]),
              "written": [str(v) for v in gold[f"{tag}_written"]], "counts": gold[f"{tag}_counts"].tolist(),
              "records": gold[f"{tag}_records"], "skipped": gold[f"{tag}_skipped"].tolist()}
        for key in gold.files:
            parts = key.split("_")
            if parts[0] != tag:
                continue
            if parts[1] == "flow":
                sc["flows"][int(parts[2])] = gold[key]
            elif parts[1] == "lod":
                sc["lods"][(int(parts[2]), int(parts[3]))] = gold[key]
            elif parts[1] == "corrected" and parts[2] == "bytes":
                sc["corrected_bytes"][int(parts[3])] = gold[key].tobytes()
            elif parts[1] == "corrected":
                sc["corrected"][int(parts[2])] = gold[key]
        out.append((tag, sc))
    return out


def coarsest_lod(scene, i, levels=5):
    for k in range(levels - 1, 0, -1):
        if (i, k) in scene["lods"]:
            return scene["lods"][(i, k)]
    return scene["flows"][i]
