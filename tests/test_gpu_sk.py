"""The SK update block on the GPU: the depthwise-convolution and GELU kernels against float64, one PCBlock through the
engine's helper, the engine with a seeded SK checkpoint against the CPU oracle of tests/mof_sk_oracle.py, its caches and
graphs in a sliding job, and that a plain checkpoint pays nothing for it.

Seed 0 throughout: tests/test_sk_cpu.py::test_every_depthwise_convolution_reaches_the_field shows, on the oracle alone, that
with it each of the twelve depthwise weights moves the field by more than the 8 N the engine is held to here."""
import pytest
import torch
import torch.nn.functional as F

from tests_support import EPE_TOL, K_OF, s16_decode

pytestmark = pytest.mark.gpu

DEPTH = 4
PATTERN = 12345.0
E24, E21 = 2.0 ** -24, 2.0 ** -21


# ----------------------------------------------------------------------------- rows in either format
def _put_rows(x, ld, off, fmt):
    """x f32 [rows, c] (host) -> a device buffer [rows][ld] filled with PATTERN, x in columns off .. off + c - 1 in format
    fmt; returns (buffer, the values the kernel will read there, float64 on the host)."""
    from vfml import hip
    rows, c = x.shape
    buf = torch.full((rows * ld,), PATTERN, device="cuda")
    if fmt == hip.FMT_S16:
        tmp = torch.empty(rows * c, device="cuda")
        hip.to_s16(x.cuda().reshape(-1).contiguous(), rows, c, c, tmp, c)
        buf.view(rows, ld)[:, off:off + c] = tmp.view(rows, c)
        seen = s16_decode(tmp, rows, c, c).double()
    else:
        buf.view(rows, ld)[:, off:off + c] = x.cuda()
        seen = x.double()
    return buf, seen


def _get_rows(buf, rows, ld, off, c, fmt):
    from vfml import hip
    v = buf.view(rows, ld)[:, off:off + c].contiguous()
    return (s16_decode(v.reshape(-1), rows, c, c) if fmt == hip.FMT_S16 else v.cpu()).double()


def _outside_untouched(buf, rows, ld, off, c):
    v = buf.view(rows, ld)
    return bool((v[:, :off] == PATTERN).all()) and bool((v[:, off + c:] == PATTERN).all())


def _gelu64(v):
    return 0.5 * v * (1 + torch.erf(v / 2 ** 0.5))


def _dw_case(n, h, w, c, k, in_fmt, out_fmt, res, act, ld_x=None, x_off=0, ld_out=None, out_off=0):
    """Largest error-to-bound ratio of hip.dwconv2d on one case.  Per-element bound, derived and not fitted:
    1.2 (k^2 + 8) 2^-24 (|x| + sum |w x| + |b|) + 8 2^-24 |y|, plus 2^-21 |y| for a split-row output: f32 accumulation of
    k^2 + 2 terms, the GELU slope of at most 1.13, erff, and the hi + lo store."""
    from vfml import hip
    g = torch.Generator().manual_seed(n * 1000 + h * 100 + c + k)
    ld_x, ld_out = ld_x or c, ld_out or c
    rows = n * h * w
    x = torch.randn(rows, c, generator=g)
    wgt = (torch.rand(c, k, k, generator=g) * 2 - 1) / k
    b = torch.rand(c, generator=g) * 2 - 1
    xbuf, seen = _put_rows(x, ld_x, x_off, in_fmt)
    obuf = torch.full((rows * ld_out,), PATTERN, device="cuda")
    hip.dwconv2d(xbuf, ld_x, n, h, w, c, k, wgt.cuda().reshape(-1).contiguous(), b.cuda(), obuf, ld_out, x_off=x_off,
                 out_off=out_off, in_fmt=in_fmt, out_fmt=out_fmt, residual=res, gelu=act)
    torch.cuda.synchronize()
    x4 = seen.view(n, h, w, c).permute(0, 3, 1, 2)
    w4 = wgt.double().view(c, 1, k, k)
    conv = F.conv2d(x4, w4, b.double(), padding=k // 2, groups=c)
    mag = x4.abs() + F.conv2d(x4.abs(), w4.abs(), None, padding=k // 2, groups=c) + b.double().abs().view(1, c, 1, 1)
    y = x4 + conv if res else conv
    y = _gelu64(y) if act else y
    bound = 1.2 * (k * k + 8) * E24 * mag + 8 * E24 * y.abs() + (E21 * y.abs() if out_fmt == hip.FMT_S16 else 0)
    got = _get_rows(obuf, rows, ld_out, out_off, c, out_fmt).view(n, h, w, c).permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    assert _outside_untouched(obuf, rows, ld_out, out_off, c)
    assert _outside_untouched(xbuf, rows, ld_x, x_off, c)
    return float(((got - y).abs() / bound).max())


SHAPES = [(2, 5, 9, 8, 15), (1, 17, 19, 40, 15), (3, 33, 70, 72, 7), (1, 16, 16, 16, 1)]


@pytest.mark.parametrize("res,act", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("in_fmt,out_fmt", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv2d_against_float64(gpu, shape, in_fmt, out_fmt, res, act):
    r = _dw_case(*shape, in_fmt, out_fmt, res, act)
    print(f"[dwconv] {shape} in {in_fmt} out {out_fmt} res {res} gelu {act}: error / bound {r:.3f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("in_fmt,out_fmt", [(0, 0), (1, 1), (1, 0)])
def test_dwconv2d_reads_and_writes_in_place_of_wider_rows(gpu, in_fmt, out_fmt):
    """24 channels read at offset 8 of rows of stride 96, written at offset 16 of rows of stride 64; the columns around both
    keep their pattern."""
    r = _dw_case(2, 11, 13, 24, 15, in_fmt, out_fmt, True, True, ld_x=96, x_off=8, ld_out=64, out_off=16)
    print(f"[dwconv] strided in {in_fmt} out {out_fmt}: error / bound {r:.3f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("rows,c", [(37, 8), (5, 976)])
def test_gelu_rows_against_float64(gpu, rows, c, inplace, fmt):
    """The depthwise bound with no taps: 1.2 * 8 * 2^-24 |x| + 8 * 2^-24 |y|, and for split rows 2^-21 |y| + 2^-25.  The
    absolute term is the storage format's, not the kernel's: |lo| <= 2^-12 |y| lies in the f16 subnormals (spacing 2^-24)
    whenever |y| < 1/4, so rounding it costs up to 2^-25 whatever y is - a correctly rounded f32 GELU of this test's very
    input, split on the CPU, is 1.22 times the bound without it (at x = -3.05e-3) and 0.30 times the bound with it.  The
    depthwise cases need no such term: there |x| + sum |w x| + |b| is of order one."""
    from vfml import hip
    x = torch.randn(rows, c, generator=torch.Generator().manual_seed(rows)) * 2
    xbuf, seen = _put_rows(x, c + 8, 8, fmt)
    obuf = xbuf if inplace else torch.full((rows * (c + 8),), PATTERN, device="cuda")
    hip.gelu_rows(xbuf, c + 8, obuf, c + 8, rows, c, x_off=8, out_off=8, in_fmt=fmt, out_fmt=fmt)
    torch.cuda.synchronize()
    y = _gelu64(seen)
    bound = 1.2 * 8 * E24 * seen.abs() + 8 * E24 * y.abs() + (E21 * y.abs() + 2.0 ** -25 if fmt == hip.FMT_S16 else 0)
    got = _get_rows(obuf, rows, c + 8, 8, c, fmt)
    r = float(((got - y).abs() / bound.clamp_min(1e-300)).max())
    print(f"[gelu_rows] {rows} x {c} fmt {fmt} in place {inplace}: error / bound {r:.3f}")
    assert r <= 1.0, r
    assert _outside_untouched(obuf, rows, c + 8, 8, c)


def test_dwconv2d_bad_arguments(gpu):
    from ctypes import c_void_p
    from vfml import hip
    n, h, w, c = 1, 6, 7, 16
    x = torch.randn(n * h * w * c, device="cuda")
    wgt = torch.randn(c * 15 * 15, device="cuda")
    b = torch.randn(c, device="cuda")
    out = torch.full((n * h * w * c,), PATTERN, device="cuda")

    def call(k=15, c=c, ld_x=c, ld_out=c, x=x, out=out, x_off=0, out_off=0, in_fmt=0, out_fmt=0):
        hip.dwconv2d(x, ld_x, n, h, w, c, k, wgt, b, out, ld_out, x_off=x_off, out_off=out_off, in_fmt=in_fmt, out_fmt=out_fmt)
    with pytest.raises(RuntimeError, match="k = 4"):
        call(k=4)
    with pytest.raises(RuntimeError, match="k = 17"):
        call(k=17)
    with pytest.raises(RuntimeError, match="x: misaligned split rows"):
        call(c=12, in_fmt=hip.FMT_S16)
    with pytest.raises(RuntimeError, match="out: misaligned split rows"):
        call(c=8, ld_out=12, out_fmt=hip.FMT_S16)
    with pytest.raises(RuntimeError, match="x: misaligned split rows"):
        call(c=8, x_off=4, in_fmt=hip.FMT_S16)
    with pytest.raises(RuntimeError, match="x: ld < c"):
        call(ld_x=8)
    with pytest.raises(RuntimeError, match="out: ld < c"):
        call(ld_out=12)
    with pytest.raises(RuntimeError, match="in place"):
        call(x=out)
    with pytest.raises(RuntimeError, match="format"):
        call(out_fmt=hip.FMT_F16)
    L = hip.lib()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    for nul in range(4):
        ptrs = [c_void_p(x.data_ptr()), c_void_p(wgt.data_ptr()), c_void_p(b.data_ptr()), c_void_p(out.data_ptr())]
        ptrs[nul] = None
        rc = L.vfml_dwconv2d(ptrs[0], c, n, h, w, c, 15, ptrs[1], ptrs[2], ptrs[3], c, 0, 0, 0, stream)
        assert rc != 0 and b"null pointer" in L.vfml_last_error()
    with pytest.raises(RuntimeError, match="null pointer"):
        hip._check(L.vfml_gelu_rows(None, c, c_void_p(out.data_ptr()), c, 4, c, 0, 0, stream), "vfml_gelu_rows")
    with pytest.raises(RuntimeError, match="out: ld < c"):
        hip.gelu_rows(x, c, out, 8, 4, c)
    with pytest.raises(RuntimeError, match="in place needs"):
        hip.gelu_rows(out, c, out, c, 4, c, in_fmt=0, out_fmt=1)
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all())


def test_torch_op_is_the_same_call(gpu):
    from vfml import hip
    import vfml.torch_ops  # noqa: F401
    n, h, w, c, k = 2, 9, 21, 24, 7
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, h, w, c, generator=g).cuda()
    wgt = (torch.randn(c, k, k, generator=g) / k).cuda()
    b = torch.randn(c, generator=g).cuda()
    out = torch.empty(n * h * w * c, device="cuda")
    hip.dwconv2d(x.reshape(-1), c, n, h, w, c, k, wgt.reshape(-1), b, out, c, residual=True, gelu=True)
    got = torch.ops.vfml.dwconv2d_nhwc(x, wgt, b, True, True)
    assert got.shape == (n, h, w, c) and torch.equal(got.reshape(-1), out)
    with pytest.raises(NotImplementedError):
        torch.ops.vfml.dwconv2d_nhwc(x.cpu(), wgt.cpu(), b.cpu(), True, True)


# ----------------------------------------------------------------------------- the engine
def _cfgs(**over):
    from oracle import mof_oracle as mo
    from vfml import get_cfg
    cfg, ocfg = get_cfg(), mo.get_cfg()
    for c in (cfg, ocfg):
        c.sk, c.decoder_depth = True, DEPTH
        for k, v in over.items():
            setattr(c, k, v)
    cfg.precision = "f16x3"
    return cfg, ocfg


def _engine(cfg, sd):
    from vfml import build_network
    net = build_network(cfg)
    net.load_state_dict(sd)
    return net.cuda().eval()


def _epe(a, b):
    return (a.double() - b.double()).pow(2).sum(2).sqrt()


def _frames(T, H, W):
    return torch.rand(1, T, 3, H, W, generator=torch.Generator().manual_seed(T * 1000 + H))


_REF = {}


def _oracle_fields(T, H, W, **over):
    """(float64 field, N = mean EPE of the float32 oracle against it) for _frames(T, H, W), once per session."""
    import mof_sk_oracle as so
    from vfml.weights import seeded_state_dict
    key = (T, H, W, tuple(sorted(over.items())))
    if key not in _REF:
        cfg, ocfg = _cfgs(**over)
        sd = seeded_state_dict(cfg, 0)
        out = []
        for dt in (torch.float32, torch.float64):
            ora = so.build_network(ocfg)
            ora.load_state_dict(sd)
            out.append(ora.eval().to(dt)(_frames(T, H, W).to(dt), {})[0])
        _REF[key] = (out[1], _epe(out[0], out[1]).mean().item())
    return _REF[key]


@pytest.mark.parametrize("name,cin,cout", [("update_block.encoder.convc1", 648, 256), ("update_block.flow_head", 128, 4)])
def test_pcblock_through_the_engines_helper(gpu, name, cin, cout):
    """One PCBlock at 17 x 19 cells against the oracle's block in float64: at most 8 times the float32 block's own deviation
    from float64 on the same input, in max and mean - and further than that from the same block with conv_list.1 transposed
    (ky <-> kx), which pins the orientation of each encoder block by itself."""
    import mof_sk_oracle as so
    from vfml import hip
    from vfml.weights import seeded_state_dict
    cfg, _ = _cfgs()
    sd = seeded_state_dict(cfg, 0)
    net = _engine(cfg, sd)
    dev = torch.device("cuda")
    P = net._pack(dev)
    h, w = 17, 19
    rows = h * w
    pos, cp, _ = net._sk_padded(name)
    x = torch.randn(rows, cin, generator=torch.Generator().manual_seed(cin))
    xp = torch.zeros(rows, cp)
    xp[:, pos] = x
    xbuf, seen = _put_rows(xp, cp, 0, hip.FMT_S16)
    seen = seen[:, pos]                                            # the input, as every side sees it
    out_fmt = hip.FMT_S16 if cout % 8 == 0 else hip.FMT_F32
    out = torch.full((rows * cout,), PATTERN, device="cuda")
    net._pcblock(name, P, xbuf, cp, 0, 1, h, w, out, cout, 0, net._sk_workspace(rows, dev), out_fmt=out_fmt)
    torch.cuda.synchronize()
    got = _get_rows(out, rows, cout, 0, cout, out_fmt)
    blk = so.PCBlock(cin, cout, (1, 15))
    blk.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")})
    x4 = seen.view(1, h, w, cin).permute(0, 3, 1, 2)
    with torch.no_grad():
        ref32 = blk(x4.float()).double()
        blk = blk.double()
        ref = blk(x4)
        blk.conv_list[1].weight.copy_(blk.conv_list[1].weight.transpose(2, 3).clone())
        wrong = blk(x4)

    def rows_of(t):
        return t[0].permute(1, 2, 0).reshape(rows, cout)
    n_max, n_mean = (ref32 - ref).abs().max().item(), (ref32 - ref).abs().mean().item()
    e = (got - rows_of(ref)).abs()
    d = (got - rows_of(wrong)).abs()
    print(f"[pcblock] {name}: engine max {e.max().item():.3e} mean {e.mean().item():.3e} | float32 block max {n_max:.3e} mean "
          f"{n_mean:.3e} | ratio max {e.max().item() / n_max:.2f} mean {e.mean().item() / n_mean:.2f} | transposed: max "
          f"{d.max().item():.3e} mean {d.mean().item():.3e}")
    assert torch.isfinite(got).all()
    assert e.max().item() <= 8 * n_max and e.mean().item() <= 8 * n_mean
    assert d.max().item() > 8 * n_max and d.mean().item() > 8 * n_mean


@pytest.mark.parametrize("T,H,W,over", [(3, 136, 152, {}), (5, 136, 152, {}), (5, 136, 152, {"network": "BOFNet"}),
                                        (3, 136, 152, {"gma": True})], ids=["mof3", "mof5", "bof5", "sk+gma3"])
def test_sk_forward_matches_oracle(gpu, T, H, W, over):
    """f16x3, depth 4, against the float64 oracle: mean EPE <= 8 N, N = the float32 oracle's own mean EPE against float64 on
    that input (nothing in the bound comes from the engine), and < EPE_TOL.  The mean alone: maximum, worst block, outer ring
    and the 1/8-resolution flows of the same fields, and a field two depthwise tiles wide, are in
    tests/test_gpu_elementwise_variants.py."""
    from vfml.weights import seeded_state_dict
    cfg, _ = _cfgs(**over)
    net = _engine(cfg, seeded_state_dict(cfg, 0))
    ref, N = _oracle_fields(T, H, W, **over)
    got, _ = net(_frames(T, H, W).cuda(), {})
    got = got.cpu()
    M = 1 if over.get("network") == "BOFNet" else T - 2
    assert got.shape == ref.shape == (1, 2 * M, 2, H, W)
    assert torch.isfinite(got).all()
    e = _epe(got, ref)
    print(f"[sk {over or 'mof'}] T={T} {H}x{W}: mean EPE {e.mean().item():.3e} px, max {e.max().item():.3e} px, N {N:.3e} px, "
          f"mean / N {e.mean().item() / N:.2f}, mean |flow| {ref.abs().mean().item():.3f} px")
    assert e.mean().item() <= K_OF["f16x3"] * N, f"mean EPE {e.mean().item():.3e} px against 8 N = {8 * N:.3e}"
    assert e.mean().item() < EPE_TOL


def _sliding_job(net, clip, passes=1):
    import contextlib
    import io
    from processing.videoflow_processor import VideoFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=5)
    proc.core.model = net
    n = clip.shape[0]
    out = []
    for _ in range(passes):
        out = [proc.compute_optical_flow_resident(clip, i).clone() for i in range(n)]
    return proc, out


def test_sk_sliding_job_is_exact(gpu):
    """test_gma_sliding_job_is_exact for an SK checkpoint at 136 x 152: all eight fields of an 8-frame job are bit-identical
    to the same windows run from scratch with empty caches, and with the graph on to the graph off.  The iteration-zero
    store is switched off for SK checkpoints: no window is warm."""
    import numpy as np
    from vfml.synth import synthetic_clip
    from vfml.weights import seeded_state_dict
    cfg, _ = _cfgs()
    sd = seeded_state_dict(cfg, 0)
    clip = torch.from_numpy(np.stack(synthetic_clip(8, 136, 152))).cuda()
    cfg.use_graph = False
    net = _engine(cfg, sd)
    proc, eager = _sliding_job(net, clip)
    assert net.iter0_stats["warm"] == 0
    for i in range(8):
        idx = list(proc.window_indices(8, i))
        net.clear_feature_cache()
        b, _ = net.forward_u8(clip[idx])
        assert torch.equal(eager[i], b[0, 3].permute(1, 2, 0)), (i, idx)
    cfg2, _ = _cfgs()
    cfg2.use_graph = True
    net2 = _engine(cfg2, sd)
    _, graphed = _sliding_job(net2, clip, passes=3)         # (a configuration is captured the second time it is seen)
    assert any(isinstance(g, torch.cuda.CUDAGraph) for g in net2._graphs.values())
    for i in range(8):
        assert torch.equal(eager[i], graphed[i]), i


@pytest.mark.parametrize("gma", [False, True])
def test_plain_checkpoint_pays_nothing(gpu, gma):
    from vfml import build_network, get_cfg
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.decoder_depth, cfg.precision, cfg.gma = DEPTH, "f16x3", gma
    assert cfg.sk is False
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    net.cuda().eval()
    net(_frames(5, 136, 152).cuda(), {})
    assert net.sk is False and not net._sk_blocks
    assert not [k for k in net._ws if k.startswith("sk_")]
    assert net._ws["gru_state"].numel() == 3 * 17 * 19 * (896 if gma else 768)
