"""ORACLE (test infrastructure, never imported by the product): numpy restatement of the turbulence map, DESIGN.md
section 10 (reference flow_visualizer.py: generate_turbulence_map :2997-3052).  OpenCV is not available, so the cv2
primitives are this project's definitions of the OpenCV 4 algorithms and nothing here is pinned against cv2:
  resize      oracle/quality_map.py resize_flow (the taps of the quality map), then the vector rescale
  boxFilter   BORDER_REFLECT, f64 window sums (prefix sums), times 1.0 / k^2, rounded once to f32
  JET         vfml/csrc/make_jet_table.py
np.percentile is numpy's own."""
import importlib.util
import os

import numpy as np

from oracle.quality_map import resize_flow

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _jet_module():
    path = os.path.join(ROOT, "video-flow-ml_amd", "vfml", "csrc", "make_jet_table.py")
    spec = importlib.util.spec_from_file_location("make_jet_table", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


JET_RGB = np.array(_jet_module().jet_table(), dtype=np.uint8)       # [256,3] RGB
JET_BGR = np.ascontiguousarray(JET_RGB[:, ::-1])


def reflect_index(n, radius):
    """Source index of positions -radius .. n-1+radius under BORDER_REFLECT (fedcba|abcdefgh|hgfedcb), periodic."""
    p = np.arange(-radius, n + radius) % (2 * n)
    return np.where(p < n, p, 2 * n - 1 - p)


def box_mean(img, k, order="rows_first"):
    """k x k box mean of a float32 image: f64 sums (exclusive prefix sums along each axis), one rounding to f32.
    `order` picks which axis is summed first - two summation orders of the same definition."""
    r = k // 2
    h, w = img.shape
    pad = img.astype(np.float64)[reflect_index(h, r)][:, reflect_index(w, r)]

    def window(a, axis):
        c = np.cumsum(a, axis=axis)
        c = np.concatenate([np.zeros_like(np.take(c, [0], axis=axis)), c], axis=axis)
        n = a.shape[axis] - k + 1
        return np.take(c, np.arange(k, k + n), axis=axis) - np.take(c, np.arange(n), axis=axis)

    s = window(window(pad, 1), 0) if order == "rows_first" else window(window(pad, 0), 1)
    return (s * (1.0 / (k * k))).astype(F)


def box_mean_direct(img, k):
    """The same by adding the k*k taps one shifted image at a time (no prefix sums): a third summation order."""
    r = k // 2
    h, w = img.shape
    pad = img.astype(np.float64)[reflect_index(h, r)][:, reflect_index(w, r)]
    s = np.zeros((h, w), np.float64)
    for dy in range(k):
        for dx in range(k):
            s += pad[dy:dy + h, dx:dx + w]
    return (s * (1.0 / (k * k))).astype(F)


def total_variation(flow, h, w, k, box=box_mean):
    """tv [h,w] float32 of a flow field [fh,fw,2]."""
    flow = np.asarray(flow, dtype=F)
    if flow.shape[:2] != (h, w):
        flow = resize_flow(flow, h, w)
    x, y = flow[..., 0], flow[..., 1]
    with np.errstate(all="ignore"):
        mx, my = box(x, k), box(y, k)
        mxx, myy = box(x * x, k), box(y * y, k)
        vx = mxx - mx * mx
        vy = myy - my * my
        return np.sqrt(np.maximum(F(0), vx) + np.maximum(F(0), vy)).astype(F)


def normalise(tv):
    """(index uint8 [h,w], lo, hi) of a tv map."""
    lo, hi = np.percentile(tv, 5), np.percentile(tv, 95)
    assert lo.dtype == F and hi.dtype == F, "numpy 2 keeps float32 percentiles of a float32 array"
    if hi - lo > F(1e-6):
        n = np.clip((tv - lo) / (hi - lo), 0, 1)
    else:
        n = np.zeros_like(tv)
    return (n * F(255)).astype(np.uint8), lo, hi


def turbulence_map(flow, h, w, k=25, box=box_mean):
    """dict(bgr uint8 [h,w,3], index uint8 [h,w], tv float32 [h,w], lohi float32 [2])."""
    tv = total_variation(flow, h, w, k, box)
    index, lo, hi = normalise(tv)
    return {"bgr": JET_BGR[index], "index": index, "tv": tv, "lohi": np.array([lo, hi], dtype=F)}


def brute_force_tv(flow, k):
    """Double loop over pixels and taps in Python floats (f64) with explicit reflection: the definition, slowly."""
    flow = np.asarray(flow, dtype=F)
    h, w = flow.shape[:2]
    r = k // 2

    def refl(p, n):
        while p < 0 or p >= n:
            p = -p - 1 if p < 0 else 2 * n - 1 - p
        return p

    tv = np.zeros((h, w), F)
    for yy in range(h):
        for xx in range(w):
            s = [0.0, 0.0, 0.0, 0.0]
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    v = flow[refl(yy + dy, h), refl(xx + dx, w)]
                    s[0] += float(v[0])
                    s[1] += float(v[1])
                    s[2] += float(v[0] * v[0])
                    s[3] += float(v[1] * v[1])
            mx, my, mxx, myy = (F(t * (1.0 / (k * k))) for t in s)
            vx, vy = F(mxx - F(mx * mx)), F(myy - F(my * my))
            tv[yy, xx] = np.sqrt(F(max(F(0), vx) + max(F(0), vy)))
    return tv


def quantised_flow(h, w, seed, scale=6.0):
    """A seeded flow field whose values are multiples of 2^-8 with |v| <= 64: every f64 window sum of the values and of
    their f32 squares is then exact (squares are multiples of 2^-16 below 2^12; f32 holds them exactly only when they fit
    24 bits, and rounds them once otherwise - either way the f64 sum of at most 63*63 of them is exact), so the result
    does not depend on the summation order.  Smooth motion plus patches of noise, so that tv has structure."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.stack([scale * np.sin(xx / 37.0 + yy / 53.0), scale * np.cos(yy / 29.0 - xx / 71.0)], axis=2)
    f += rng.normal(0, 1, (h, w, 2)) * rng.choice([0.0, 0.05, 0.5, 3.0], (max(1, (h + 15) // 16), max(1, (w + 15) // 16), 1)
                                                  ).repeat(16, 0).repeat(16, 1)[:h, :w]
    return (np.clip(np.round(f * 256.0), -64 * 256, 64 * 256) / 256.0).astype(F)
