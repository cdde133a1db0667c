"""forward_interpolate in numpy (TEST INFRASTRUCTURE ONLY): the definition of DESIGN.md section 19, which
vfml_flow_forward_interpolate is held to bit for bit.

    source cell s = (xs, ys), row-major index ys * w + xs, lands at  x1 = xs + f.x,  y1 = ys + f.y
    s is valid iff  0 < x1 < w  and  0 < y1 < h          (strict, as RAFT's forward_interpolate; NaN and infinities fail)
    target (x, y):  d2 = (x1 - x) * (x1 - x) + (y1 - y) * (y1 - y);  the result is f[s*], s* the valid source of least d2,
                    ties to the LOWEST source index; zero everywhere when no source is valid

Every operation is done in the flow's own dtype (float32: numpy rounds each operation on its own, nothing is fused;
float64 for the float64 oracle stream), and argmin returns the first minimum, which is the lowest index.  The mutants
(`strict`, `tie`) and the two other readings (`backward_warp`, `no_hole_filling`) exist so that the CPU tests can show that the
fixtures tell the definition from its nearest misreadings."""
import numpy as np


def landing(flow, strict=True):
    """flow [h, w, 2] -> (x1 [P], y1 [P], valid [P]) in the flow's dtype, sources in row-major order."""
    h, w = flow.shape[:2]
    dt = flow.dtype
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore", over="ignore"):
        x1 = (xs.astype(dt) + flow[..., 0]).reshape(-1)
        y1 = (ys.astype(dt) + flow[..., 1]).reshape(-1)
        if strict:
            valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
        else:
            valid = (x1 >= 0) & (x1 < w) & (y1 >= 0) & (y1 < h)
    return x1, y1, valid


def forward_interpolate(flow, targets=None, strict=True, tie="lowest", chunk_elems=1 << 24):
    """flow [h, w, 2] (float32 or float64) -> (out, index, margin) for the target cells `targets` (flat row-major indices;
    None: every cell, and the three results come back as [h, w, 2], [h, w] and [h, w]):
        out     [n, 2]  flow[s*] in the flow's dtype (zero where no source is valid)
        index   [n]     int32 s*, -1 where no source is valid
        margin  [n]     float64: distance (cells, not squared) to the second-best valid source minus the distance to the best,
                        from the landing points as computed in the flow's dtype; inf with fewer than two valid sources
    The targets are walked in chunks of at most chunk_elems / P rows of the distance matrix."""
    flow = np.ascontiguousarray(flow)
    h, w = flow.shape[:2]
    dt = flow.dtype
    P = h * w
    x1, y1, valid = landing(flow, strict)
    src = np.flatnonzero(valid)                    # rising source index: argmin's first minimum is the lowest index
    full = targets is None
    tg = np.arange(P) if full else np.asarray(targets).reshape(-1)
    n = len(tg)
    out = np.zeros((n, 2), dt)
    index = np.full(n, -1, np.int32)
    margin = np.full(n, np.inf, np.float64)
    if len(src):
        sx, sy = x1[src], y1[src]
        if tie == "highest":
            src, sx, sy = src[::-1], sx[::-1], sy[::-1]
        elif tie != "lowest":
            raise ValueError(tie)
        f2 = flow.reshape(P, 2)
        rows = max(1, chunk_elems // len(src))
        for a in range(0, n, rows):
            t = tg[a:a + rows]
            tx, ty = (t % w).astype(dt)[:, None], (t // w).astype(dt)[:, None]
            dx, dy = sx[None, :] - tx, sy[None, :] - ty
            d2 = dx * dx + dy * dy                                   # three roundings in dt, no fused multiply-add
            k = np.argmin(d2, axis=1)
            index[a:a + rows] = src[k]
            out[a:a + rows] = f2[src[k]]
            if len(src) > 1:
                d = np.sqrt(d2.astype(np.float64))
                best = d[np.arange(len(t)), k].copy()
                d[np.arange(len(t)), k] = np.inf
                margin[a:a + rows] = d.min(axis=1) - best
    if full:
        return out.reshape(h, w, 2), index.reshape(h, w), margin.reshape(h, w)
    return out, index, margin


def backward_warp(flow):
    """A misreading: the gather  out(x, y) = f(round(x - f.x), round(y - f.y))  clamped to the frame."""
    h, w = flow.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore"):
        gx = np.clip(np.nan_to_num(np.rint(xs - flow[..., 0])), 0, w - 1).astype(np.int64)
        gy = np.clip(np.nan_to_num(np.rint(ys - flow[..., 1])), 0, h - 1).astype(np.int64)
    return flow[gy, gx]


def no_hole_filling(flow):
    """A misreading: every valid source is splatted onto the cell nearest to its landing point (lowest index wins), cells
    nobody lands on stay zero."""
    h, w = flow.shape[:2]
    x1, y1, valid = landing(flow)
    out = np.zeros_like(flow)
    f2 = flow.reshape(-1, 2)
    for s in np.flatnonzero(valid)[::-1]:
        x, y = int(np.rint(x1[s])), int(np.rint(y1[s]))
        if 0 <= x < w and 0 <= y < h:
            out[y, x] = f2[s]
    return out


# ----------------------------------------------------------------------------- fixtures
def fixture(kind, h, w, seed=0):
    """The named input flows [h, w, 2] float32 of the CPU and GPU tests."""
    g = np.random.default_rng(seed * 1000003 + h * 1009 + w)
    f = np.zeros((h, w, 2), np.float32)
    if kind == "zero":
        return f
    if kind.startswith("uniform"):                 # "uniform:1,-2" integer, "uniform:0.5,0" half-integer (exact ties)
        fx, fy = (float(v) for v in kind.split(":")[1].split(","))
        f[..., 0], f[..., 1] = fx, fy
        return f
    if kind.startswith("sigma"):                   # "sigma0.5", "sigma3", "sigma20"
        return (g.standard_normal((h, w, 2)) * float(kind[5:])).astype(np.float32)
    if kind == "nonfinite":                        # sigma 1 with NaN and +-inf entries
        f = g.standard_normal((h, w, 2)).astype(np.float32)
        flat = f.reshape(-1)
        at = g.permutation(flat.size)[:max(3, flat.size // 5)]
        flat[at[0::3]] = np.nan
        flat[at[1::3]] = np.inf
        flat[at[2::3]] = -np.inf
        return f
    if kind == "all_invalid":                      # every source leaves the frame to the left
        f[..., 0] = -float(w) - 1.0
        f[..., 1] = 0.25
        return f
    if kind == "one_valid":                        # all leave but one cell, whose value must appear everywhere
        f[..., 0] = -float(w) - 1.0
        y, x = h // 2, w // 3
        f[y, x] = (0.25, 0.375)
        return f
    if kind == "duplicate":                        # two sources on one landing point with different values; the rest leave
        f[..., 0] = -float(w) - 1.0
        if h * w < 3:                             # (nothing to duplicate: the one cell stays)
            f[0, 0] = (0.25, 0.5)
        elif w >= 3:
            f[h // 2, 0] = (1.5, 0.5)              # lands at (1.5, h//2 + 0.5)
            f[h // 2, 2] = (-0.5, 0.5)             # lands at (1.5, h//2 + 0.5): the same point, another value
        else:                                      # a one-column grid: the same along y
            f[...] = (0.5, -float(h) - 1.0)
            f[0, 0] = (0.5, 1.5)
            f[2, 0] = (0.5, -0.5)
        return f
    raise ValueError(kind)


FIXTURES = ("zero", "uniform:1,-2", "uniform:-3,2", "uniform:0.5,0", "uniform:0.5,0.5", "uniform:-1.5,2.5", "sigma0.5", "sigma3",
            "sigma20", "nonfinite", "all_invalid", "one_valid", "duplicate")
