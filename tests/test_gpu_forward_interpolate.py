"""vfml_flow_forward_interpolate against the numpy definition (tests/forward_interpolate_oracle.py): values AND chosen source
indices, bit for bit, on every fixture of tests/test_forward_interpolate_cpu.py.

The kernel as built (csrc/warm_start.hip): a workgroup owns FI_TARGETS = 256 target cells and one chunk of FI_CHUNK = 2048 source
cells, staged through LDS in tiles of FI_TILE = 256.  Grids: 1x1, 1x7, 5x1 (degenerate), 16x24, 17x19 (323 cells: ragged in
every tile), 32x33 (1056 cells: five target tiles, one chunk) and 45x47 = 2115 cells - more than one source tile and more than
one source chunk, a multiple of neither (2115 = 8 * 256 + 67 = 2048 + 67): two chunks, the second of 67 sources, whose partial
minima the second pass combines."""
import ctypes

import numpy as np
import pytest
import torch

import forward_interpolate_oracle as fio

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1), (1, 7), (5, 1), (16, 24), (17, 19), (32, 33), (45, 47)]
CANARY = 12345.0


def _call(flows, ld_in=2, ld_out=2, index=True):
    """flows: [n] arrays [h, w, 2] -> (out [n, h, w, ld_out], index [n, h, w] or None) through hip.flow_forward_interpolate;
    pad channels of the input and the whole output start as a canary."""
    from vfml import hip
    n, (h, w) = len(flows), flows[0].shape[:2]
    src = np.full((n, h, w, ld_in), CANARY, np.float32)
    for k, f in enumerate(flows):
        src[k, ..., :2] = f
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((n, h, w, ld_out), CANARY, device="cuda")
    d_idx = torch.full((n, h, w), -7, dtype=torch.int32, device="cuda") if index else None
    got = hip.flow_forward_interpolate(d_in.view(-1), h, w, n=n, ld_in=ld_in, out=d_out.view(-1), ld_out=ld_out,
                                       index=None if d_idx is None else d_idx.view(-1))
    assert got.data_ptr() == d_out.data_ptr()
    return d_out.cpu().numpy(), None if d_idx is None else d_idx.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


@pytest.mark.parametrize("h,w", GRIDS, ids=[f"{h}x{w}" for h, w in GRIDS])
def test_every_fixture_bit_for_bit(gpu, h, w):
    for kind in fio.FIXTURES:
        f = fio.fixture(kind, h, w)
        want, want_idx, _ = fio.forward_interpolate(f)
        out, idx = _call([f])
        bad = int((idx[0] != want_idx).sum())
        assert bad == 0, f"{kind} {h}x{w}: {bad} cells choose another source"
        assert _same_bits(out[0], want), f"{kind} {h}x{w}: values differ"


def test_three_maps_in_one_call_stay_independent(gpu):
    h, w = 45, 47
    kinds = ("sigma3", "all_invalid", "uniform:0.5,0.5")
    flows = [fio.fixture(k, h, w) for k in kinds]
    out, idx = _call(flows, ld_in=4, ld_out=4)
    for k, f in enumerate(flows):
        want, want_idx, _ = fio.forward_interpolate(f)
        assert np.array_equal(idx[k], want_idx), kinds[k]
        assert _same_bits(out[k, ..., :2], want), kinds[k]
    assert not out[..., 2:].any()                                       # channels 2..3 of a 4-wide output: written as zero


@pytest.mark.parametrize("ld_in,ld_out", [(2, 2), (2, 4), (4, 2), (4, 4)])
def test_row_strides(gpu, ld_in, ld_out):
    h, w = 17, 19
    f = fio.fixture("sigma3", h, w)
    want, want_idx, _ = fio.forward_interpolate(f)
    out, idx = _call([f], ld_in, ld_out)
    assert np.array_equal(idx[0], want_idx) and _same_bits(out[0, ..., :2], want)
    if ld_out == 4:
        assert not out[..., 2:].any()
    out2, none = _call([f], ld_in, ld_out, index=False)                 # the index map is optional
    assert none is None and _same_bits(out2, out)


def test_1080p_sampled_cells_and_run_to_run_identity(gpu):
    """135 x 240 = 32400 cells, 16 chunks, sigma = 3: 2000 sampled target cells against the oracle (computed in row chunks), the
    index map's range over the whole grid, and two calls that agree in every bit."""
    h, w = 135, 240
    f = fio.fixture("sigma3", h, w)
    out, idx = _call([f], ld_in=4, ld_out=4)
    t = np.random.default_rng(1).permutation(h * w)[:2000]
    t[:4] = (0, w - 1, h * w - w, h * w - 1)
    want, want_idx, _ = fio.forward_interpolate(f, targets=t)
    assert np.array_equal(idx.reshape(-1)[t], want_idx)
    assert _same_bits(out.reshape(-1, 4)[t, :2], want)
    _, _, valid = fio.landing(f)
    flat = idx.reshape(-1)
    assert flat.min() >= 0 and flat.max() < h * w and valid[flat].all()             # every cell: a valid source of the grid
    assert _same_bits(out.reshape(-1, 4)[:, :2], f.reshape(-1, 2)[flat]) and not out[..., 2:].any()
    out2, idx2 = _call([f], ld_in=4, ld_out=4)
    assert _same_bits(out, out2) and np.array_equal(idx, idx2)


def test_bad_arguments_launch_nothing(gpu):
    from vfml import hip
    L = hip.lib()
    h, w = 17, 19
    P = h * w
    flow = torch.zeros(P * 4, device="cuda")
    out = torch.full((P * 4,), CANARY, device="cuda")
    ws = hip.flow_forward_interpolate_workspace(1, h, w, "cuda")
    assert L.vfml_flow_forward_interpolate_workspace_bytes(1, h, w) == 8 * P
    assert L.vfml_flow_forward_interpolate_workspace_bytes(3, 45, 47) == 3 * 2 * 2115 * 8
    assert L.vfml_flow_forward_interpolate_workspace_bytes(1, 0, w) == 0
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(fl=p(flow), ld_in=4, n=1, hh=h, ww=w, o=p(out), ld_out=4, idx=None, wsp=p(ws), wsb=ws.numel() * 8):
        return L.vfml_flow_forward_interpolate(fl, ld_in, n, hh, ww, o, ld_out, idx, wsp, wsb, st)

    for kw, text in ((dict(fl=None), b"null pointer"), (dict(o=None), b"null pointer"), (dict(wsp=None), b"null pointer"),
                     (dict(n=0), b"n = 0"), (dict(hh=0), b"h = 0"), (dict(ww=-1), b"w = -1"), (dict(hh=4097, ww=4097), b"2^24"),
                     (dict(ld_in=1), b"ld_in = 1"), (dict(ld_out=1), b"ld_out = 1"),
                     (dict(wsb=8 * P - 8), b"workspace"), (dict(wsp=p(ws, 4)), b"workspace"), (dict(n=2), b"workspace"),
                     (dict(fl=p(flow, 2)), b"alignment"), (dict(o=p(flow)), b"overlaps"), (dict(o=p(flow, 16)), b"overlaps")):
        assert call(**kw) != 0, kw
        assert text in L.vfml_last_error(), (kw, L.vfml_last_error())
    with pytest.raises(ValueError, match="flow holds"):
        hip.flow_forward_interpolate(flow, h, w, n=2, ld_in=4)
    with pytest.raises(ValueError, match="expected"):
        hip.flow_forward_interpolate(torch.zeros(3, 5, device="cuda"))
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    assert call() == 0                                                  # ... and the good call still runs
    torch.cuda.synchronize()
    assert not bool(out.any())
