"""The Twins-SVT encoders on the GPU: the three new kernels against float64 restatements, one encoder
through the engine's helper, the engine with seeded Twins checkpoints against the CPU oracle of tests/mof_twins_oracle.py, its
caches and graphs in a sliding job, and that other checkpoints pay nothing for it.

Yardstick of the kernel tests: the error against a float64 PyTorch restatement on the values the kernel actually reads (split
rows decoded as tests/test_gpu_sk.py::_put_rows does) is at most 8 times the float32 PyTorch op's own deviation from float64
on that input, in maximum and in mean; a split-row output adds its storage term 2^-21 |y| + 2^-25
(tests/test_gpu_sk.py::test_gelu_rows_against_float64 derives it).  Nothing in a bound comes from the engine."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_sk import PATTERN, _get_rows, _outside_untouched, _put_rows
from tests_support import EPE_TOL, K_OF, assert_within, error_stats, noise_floor, s16_decode

pytestmark = pytest.mark.gpu

DEPTH = 4
K = 8.0
FMTS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _check(what, got, ref64, ref32, out_fmt):
    """got, ref64, ref32: float64 tensors of one shape.  Prints the figures, then asserts max and mean."""
    from vfml import hip
    e = (got - ref64).abs()
    n = (ref32 - ref64).abs()
    store = (2.0 ** -21 * ref64.abs() + 2.0 ** -25) if out_fmt == hip.FMT_S16 else torch.zeros_like(ref64)
    b_max, b_mean = K * n.max().item() + store.max().item(), K * n.mean().item() + store.mean().item()
    # (one key: the float32 op is exact, the bound is zero and so must the error be)
    print(f"[{what}] error max {e.max().item():.3e} mean {e.mean().item():.3e} | float32 op max {n.max().item():.3e} mean "
          f"{n.mean().item():.3e} | bound max {b_max:.3e} mean {b_mean:.3e} | ratio max {e.max().item() / max(b_max, 1e-300):.2f} "
          f"mean {e.mean().item() / max(b_mean, 1e-300):.2f}")
    assert torch.isfinite(got).all()
    assert e.max().item() <= b_max and e.mean().item() <= b_mean
    return b_max, b_mean


# ----------------------------------------------------------------------------- layernorm_rows
def _ln_case(rows, c, in_fmt, out_fmt, ld=None, off=0, inplace=False, x=None):
    from vfml import hip
    g = torch.Generator().manual_seed(rows * 7 + c)
    if x is None:
        x = torch.randn(rows, c, generator=g) * 1.5 + 0.3
    gamma = 0.75 + 0.5 * torch.rand(c, generator=g)
    beta = 0.2 * torch.rand(c, generator=g) - 0.1
    ld = ld or c
    xbuf, seen = _put_rows(x, ld, off, in_fmt)
    obuf = xbuf if inplace else torch.full((rows * ld,), PATTERN, device="cuda")
    hip.layernorm_rows(xbuf, ld, obuf, ld, rows, c, gamma.cuda(), beta.cuda(), x_off=off, out_off=off, in_fmt=in_fmt, out_fmt=out_fmt)
    torch.cuda.synchronize()
    ref64 = F.layer_norm(seen, (c,), gamma.double(), beta.double(), 1e-5)
    ref32 = F.layer_norm(seen.float(), (c,), gamma, beta, 1e-5).double()
    got = _get_rows(obuf, rows, ld, off, c, out_fmt)
    assert _outside_untouched(obuf, rows, ld, off, c)
    _check(f"layernorm {rows}x{c} in {in_fmt} out {out_fmt} ld {ld} off {off} in place {inplace}", got, ref64, ref32, out_fmt)


@pytest.mark.parametrize("in_fmt,out_fmt", FMTS)
@pytest.mark.parametrize("rows,c", [(37, 128), (5, 256), (1000, 128),
                                    # what the entry point accepts beyond the encoders' own widths: a row is held by G = 16,
                                    # 32 or 64 lanes (c / 8 units up to 16, up to 32, above), in up to four passes of G units
                                    (37, 8),        # G = 16 with one lane live
                                    (37, 136),      # 17 units: G = 32, half of it without channels
                                    (37, 264),      # 33 units: G = 64 in one pass, ragged
                                    (21, 520),      # 65 units: G = 64, a second pass with one live lane
                                    (9, 2048)])     # LN_MAX_C: all four passes full
def test_layernorm_rows_against_float64(gpu, rows, c, in_fmt, out_fmt):
    _ln_case(rows, c, in_fmt, out_fmt)


@pytest.mark.parametrize("fmt", [0, 1])
def test_layernorm_rows_in_place_and_in_a_slice(gpu, fmt):
    """In place; and 128 channels at offset 8 of rows 16 wider than c, the columns around them keeping their pattern.  The
    same at c = 520 (G = 64, a second pass with one live lane: the last lane's store is the one next to the pattern)."""
    _ln_case(37, 128, fmt, fmt, inplace=True)
    _ln_case(37, 128, fmt, fmt, ld=144, off=8)
    _ln_case(37, 128, fmt, fmt, ld=144, off=8, inplace=True)
    _ln_case(21, 520, fmt, fmt, ld=536, off=8)
    _ln_case(21, 520, fmt, fmt, ld=536, off=8, inplace=True)


@pytest.mark.parametrize("fmt", [0, 1])
def test_layernorm_rows_far_from_zero(gpu, fmt):
    """Rows whose |mean| is 100 times their spread: E[x^2] - E[x]^2 in f32 would lose the variance's leading digits.  At
    c = 256 (G = 32, every lane full) and at c = 520 (G = 64, two passes, the mean folded over lanes without channels)."""
    for c in (256, 520):
        g = torch.Generator().manual_seed(5)
        x = 100.0 * (torch.rand(37, 1, generator=g) + 0.5) * torch.tensor([1.0, -1.0])[torch.arange(37) % 2].view(37, 1) \
            + torch.randn(37, c, generator=g)
        _ln_case(37, c, fmt, fmt, x=x)


# ----------------------------------------------------------------------------- window_attention
def _window_ref(qkv, pad_row, n, h, w, c, heads, masked=False):
    """qkv [n*h*w, 3c], pad_row [3c] (one dtype) -> [n*h*w, c]: the definition, restated (windows of 7 anchored at (0, 0),
    positions outside the grid hold pad_row and are keys like any other - or, `masked`, are not)."""
    ws, d = 7, 32
    ph, pw = -h % ws, -w % ws
    Hp, Wp = h + ph, w + pw
    g = pad_row.view(1, 1, 1, 3 * c).expand(n, Hp, Wp, 3 * c).clone()
    g[:, :h, :w] = qkv.view(n, h, w, 3 * c)
    real = torch.zeros(Hp, Wp, dtype=torch.bool)
    real[:h, :w] = True
    gh, gw = Hp // ws, Wp // ws
    t = g.view(n, gh, ws, gw, ws, 3, heads, d).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, n, gh, gw, heads, ws * ws, d)
    s = (t[0] @ t[1].transpose(-2, -1)) / d ** 0.5
    if masked:
        keep = real.view(gh, ws, gw, ws).permute(0, 2, 1, 3).reshape(1, gh, gw, 1, 1, ws * ws)
        s = s.masked_fill(~keep, float("-inf"))
    o = s.softmax(-1) @ t[2]                                                   # [n, gh, gw, heads, 49, d]
    o = o.view(n, gh, gw, heads, ws, ws, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(n, Hp, Wp, c)
    return o[:, :h, :w].reshape(n * h * w, c)


@pytest.mark.parametrize("in_fmt,out_fmt", [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("shape", [(2, 5, 9, 128, 4), (1, 17, 19, 256, 8), (1, 14, 21, 128, 4)], ids=lambda s: "x".join(map(str, s)))
def test_window_attention_against_float64(gpu, shape, in_fmt, out_fmt):
    """One window row padded both ways; 3 x 3 windows with ragged last ones; no padding.  A non-zero pad_row; on the padded
    shapes the result is farther than the bound from the restatement with the pad keys masked."""
    from vfml import hip
    n, h, w, c, heads = shape
    g = torch.Generator().manual_seed(h * 100 + w)
    rows = n * h * w
    qkv = torch.randn(rows, 3 * c, generator=g)
    pad_row = torch.randn(3 * c, generator=g)
    ld, off, ldo, ooff = 3 * c + 16, 8, c + 8, 8
    qbuf, seen = _put_rows(qkv, ld, off, in_fmt)
    obuf = torch.full((rows * ldo,), PATTERN, device="cuda")
    hip.window_attention(qbuf, ld, n, h, w, c, heads, 7, pad_row.cuda(), obuf, ldo, qkv_off=off, out_off=ooff, in_fmt=in_fmt,
                         out_fmt=out_fmt)
    torch.cuda.synchronize()
    ref64 = _window_ref(seen, pad_row.double(), n, h, w, c, heads)
    ref32 = _window_ref(seen.float(), pad_row, n, h, w, c, heads).double()
    got = _get_rows(obuf, rows, ldo, ooff, c, out_fmt)
    assert _outside_untouched(obuf, rows, ldo, ooff, c) and _outside_untouched(qbuf, rows, ld, off, 3 * c)
    b_max, b_mean = _check(f"window_attention {shape} in {in_fmt} out {out_fmt}", got, ref64, ref32, out_fmt)
    if h % 7 or w % 7:
        d = (got - _window_ref(seen, pad_row.double(), n, h, w, c, heads, masked=True)).abs()
        print(f"[window_attention {shape}] from the pad-masked restatement: max {d.max().item():.3e} mean {d.mean().item():.3e}")
        assert d.max().item() > b_max and d.mean().item() > b_mean


# ----------------------------------------------------------------------------- attention_shared_keys
def _shared_ref(q, kv, n, p, pk, c, heads):
    d = 32
    qh = q.view(n, p, heads, d).transpose(1, 2)
    k = kv.view(n, pk, 2, heads, d)[:, :, 0].transpose(1, 2)
    v = kv.view(n, pk, 2, heads, d)[:, :, 1].transpose(1, 2)
    o = ((qh @ k.transpose(-2, -1)) / d ** 0.5).softmax(-1) @ v
    return o.transpose(1, 2).reshape(n * p, c)


def _shared_case(shape, q_fmt, kv_fmt, out_fmt, q_scale=1.0):
    from vfml import hip
    n, p, pk, c, heads = shape
    g = torch.Generator().manual_seed(p + pk)
    q = torch.randn(n * p, c, generator=g) * q_scale
    kv = torch.randn(n * pk, 2 * c, generator=g)
    ldq, ldkv, ldo = c + 8, 2 * c + 16, c + 16
    qbuf, qs = _put_rows(q, ldq, 8, q_fmt)
    kbuf, ks = _put_rows(kv, ldkv, 8, kv_fmt)
    obuf = torch.full((n * p * ldo,), PATTERN, device="cuda")
    hip.attention_shared_keys(qbuf, ldq, kbuf, ldkv, n, p, pk, c, heads, obuf, ldo, q_off=8, kv_off=8, out_off=8, q_fmt=q_fmt,
                              kv_fmt=kv_fmt, out_fmt=out_fmt)
    torch.cuda.synchronize()
    ref64 = _shared_ref(qs, ks, n, p, pk, c, heads)
    ref32 = _shared_ref(qs.float(), ks.float(), n, p, pk, c, heads).double()
    got = _get_rows(obuf, n * p, ldo, 8, c, out_fmt)
    assert _outside_untouched(obuf, n * p, ldo, 8, c)
    _check(f"attention_shared_keys {shape} q {q_fmt} kv {kv_fmt} out {out_fmt} q x {q_scale:g}", got, ref64, ref32, out_fmt)


SHARED = [(2, 1292, 16, 128, 4), (1, 323, 300, 256, 8), (1, 70, 2040, 128, 4), (1, 64, 1, 128, 4)]


@pytest.mark.parametrize("q_fmt,kv_fmt,out_fmt", [(0, 0, 0), (0, 0, 1), (1, 1, 1)])
@pytest.mark.parametrize("shape", SHARED, ids=lambda s: "x".join(map(str, s)))
def test_attention_shared_keys_against_float64(gpu, shape, q_fmt, kv_fmt, out_fmt):
    """The test frame's own shape; pk no multiple of any chunk; the workload's key count (several LDS chunks) with few
    queries; one key."""
    _shared_case(shape, q_fmt, kv_fmt, out_fmt)


def test_attention_shared_keys_large_scores(gpu):
    """q times 8.5: scores q . k / sqrt 32 reach about +-40 (printed, and asserted beyond +-30); softmax weights computed as
    exp(s) / sum exp(s) without the running maximum lose the small scores' rows to underflow and the large ones' to
    overflow."""
    n, p, pk, c, heads = shape = (1, 323, 300, 256, 8)
    g = torch.Generator().manual_seed(p + pk)
    q = torch.randn(n * p, c, generator=g) * 8.5
    kv = torch.randn(n * pk, 2 * c, generator=g)
    s = (q.view(p, heads, 32).transpose(0, 1) @ kv.view(pk, 2, heads, 32)[:, 0].permute(1, 2, 0)) / 32 ** 0.5
    print(f"[attention_shared_keys] scores: max {s.max().item():.1f} min {s.min().item():.1f} std {s.std().item():.1f}")
    assert s.max().item() > 30 and s.min().item() < -30
    _shared_case(shape, 0, 0, 0, q_scale=8.5)


def test_attention_shared_keys_frames_do_not_mix(gpu):
    from vfml import hip
    n, p, pk, c, heads = 2, 200, 150, 128, 4
    g = torch.Generator().manual_seed(9)
    q = torch.randn(n * p * c, generator=g).cuda()
    kv = torch.randn(n * pk * 2 * c, generator=g).cuda()
    a, b = torch.empty(n * p * c, device="cuda"), torch.empty(n * p * c, device="cuda")
    hip.attention_shared_keys(q, c, kv, 2 * c, n, p, pk, c, heads, a, c)
    kv2 = kv.clone()
    kv2[pk * 2 * c:] = torch.randn(pk * 2 * c, generator=g).cuda()
    hip.attention_shared_keys(q, c, kv2, 2 * c, n, p, pk, c, heads, b, c)
    torch.cuda.synchronize()
    assert torch.equal(a[:p * c], b[:p * c])
    assert not torch.equal(a[p * c:], b[p * c:])


# ----------------------------------------------------------------------------- bad arguments
def test_twins_kernels_bad_arguments(gpu):
    from ctypes import c_void_p
    from vfml import hip
    c, heads = 128, 4
    x = torch.randn(64 * 3 * c, device="cuda")
    gam = torch.randn(c, device="cuda")
    pad = torch.randn(3 * c, device="cuda")
    out = torch.full((64 * 3 * c,), PATTERN, device="cuda")
    with pytest.raises(RuntimeError, match="vfml_layernorm_rows: bad shape"):
        hip.layernorm_rows(x, c, out, c, 8, 12, gam, gam)
    with pytest.raises(RuntimeError, match="x: ld < c"):
        hip.layernorm_rows(x, 64, out, c, 8, c, gam, gam)
    with pytest.raises(RuntimeError, match="out: misaligned split rows"):
        hip.layernorm_rows(x, c, out, c, 8, c, gam, gam, out_off=4, out_fmt=hip.FMT_S16)
    with pytest.raises(RuntimeError, match="format"):
        hip.layernorm_rows(x, c, out, c, 8, c, gam, gam, in_fmt=hip.FMT_F16)
    with pytest.raises(RuntimeError, match="in place needs"):
        hip.layernorm_rows(out, c, out, 2 * c, 8, c, gam, gam)
    with pytest.raises(RuntimeError, match="ws = 8"):
        hip.window_attention(x, 3 * c, 1, 7, 7, c, heads, 8, pad, out, c)
    with pytest.raises(RuntimeError, match="is not heads \\* 32"):
        hip.window_attention(x, 3 * c, 1, 7, 7, c, 3, 7, pad, out, c)
    with pytest.raises(RuntimeError, match="qkv: ld < 3 c"):
        hip.window_attention(x, 2 * c, 1, 7, 7, c, heads, 7, pad, out, c)
    with pytest.raises(RuntimeError, match="out: ld < c"):
        hip.window_attention(x, 3 * c, 1, 7, 7, c, heads, 7, pad, out, 64)
    with pytest.raises(RuntimeError, match="qkv: misaligned split rows"):
        hip.window_attention(x, 3 * c, 1, 7, 7, c, heads, 7, pad, out, c, qkv_off=4, in_fmt=hip.FMT_S16)
    with pytest.raises(RuntimeError, match="pk = 0"):
        hip.attention_shared_keys(x, c, x, 2 * c, 1, 16, 0, c, heads, out, c)
    with pytest.raises(RuntimeError, match="is not heads \\* 32"):
        hip.attention_shared_keys(x, c, x, 2 * c, 1, 16, 4, c, 5, out, c)
    with pytest.raises(RuntimeError, match="q: ld < c"):
        hip.attention_shared_keys(x, 64, x, 2 * c, 1, 16, 4, c, heads, out, c)
    with pytest.raises(RuntimeError, match="kv: ld < 2 c"):
        hip.attention_shared_keys(x, c, x, c, 1, 16, 4, c, heads, out, c)
    with pytest.raises(RuntimeError, match="kv: misaligned split rows"):
        hip.attention_shared_keys(x, c, x, 2 * c, 1, 16, 4, c, heads, out, c, kv_off=4, kv_fmt=hip.FMT_S16)
    with pytest.raises(RuntimeError, match="in place"):
        hip.attention_shared_keys(out, c, x, 2 * c, 1, 16, 4, c, heads, out, c)
    L = hip.lib()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    px, pg, pp, po = (c_void_p(t.data_ptr()) for t in (x, gam, pad, out))
    for nul in range(4):
        a = [px, po, pg, pg]
        a[nul] = None
        assert L.vfml_layernorm_rows(a[0], c, a[1], c, 8, c, a[2], a[3], 1e-5, 0, 0, stream) != 0
        assert b"vfml_layernorm_rows: null pointer" in L.vfml_last_error()
    for nul in range(3):
        a = [px, pp, po]
        a[nul] = None
        assert L.vfml_window_attention(a[0], 3 * c, 1, 7, 7, c, heads, 7, a[1], a[2], c, 0, 0, stream) != 0
        assert b"vfml_window_attention: null pointer" in L.vfml_last_error()
        a = [px, px, po]
        a[nul] = None
        assert L.vfml_attention_shared_keys(a[0], c, a[1], 2 * c, 1, 16, 4, c, heads, a[2], c, 0, 0, 0, stream) != 0
        assert b"vfml_attention_shared_keys: null pointer" in L.vfml_last_error()
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all())


def test_torch_ops_are_the_same_calls(gpu):
    from vfml import hip
    import vfml.torch_ops  # noqa: F401
    g = torch.Generator().manual_seed(4)
    rows, c, heads = 50, 128, 4
    x = torch.randn(rows, c, generator=g).cuda()
    gam, bet = torch.randn(c, generator=g).cuda(), torch.randn(c, generator=g).cuda()
    out = torch.empty(rows * c, device="cuda")
    hip.layernorm_rows(x.reshape(-1), c, out, c, rows, c, gam, bet)
    assert torch.equal(torch.ops.vfml.layernorm_rows(x, gam, bet, 1e-5).reshape(-1), out)
    n, h, w = 2, 9, 10
    qkv = torch.randn(n, h, w, 3 * c, generator=g).cuda()
    pad = torch.randn(3 * c, generator=g).cuda()
    out = torch.empty(n * h * w * c, device="cuda")
    hip.window_attention(qkv.reshape(-1), 3 * c, n, h, w, c, heads, 7, pad, out, c)
    got = torch.ops.vfml.window_attention(qkv, pad, heads)
    assert got.shape == (n, h, w, c) and torch.equal(got.reshape(-1), out)
    p, pk = 90, 70
    q, kv = torch.randn(n, p, c, generator=g).cuda(), torch.randn(n, pk, 2 * c, generator=g).cuda()
    out = torch.empty(n * p * c, device="cuda")
    hip.attention_shared_keys(q.reshape(-1), c, kv.reshape(-1), 2 * c, n, p, pk, c, heads, out, c)
    got = torch.ops.vfml.attention_shared_keys(q, kv, heads)
    assert got.shape == (n, p, c) and torch.equal(got.reshape(-1), out)
    with pytest.raises(NotImplementedError):
        torch.ops.vfml.layernorm_rows(x.cpu(), gam.cpu(), bet.cpu(), 1e-5)
    with pytest.raises(NotImplementedError):
        torch.ops.vfml.window_attention(qkv.cpu(), pad.cpu(), heads)
    with pytest.raises(NotImplementedError):
        torch.ops.vfml.attention_shared_keys(q.cpu(), kv.cpu(), heads)


# ----------------------------------------------------------------------------- the engine
def _cfgs(**over):
    from oracle import mof_oracle as mo
    from vfml import get_cfg
    cfg, ocfg = get_cfg(), mo.get_cfg()
    for c in (cfg, ocfg):
        c.twins, c.decoder_depth = True, DEPTH
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


@pytest.mark.parametrize("prefix", ["fnet", "cnet"])
def test_twins_encoder_through_the_engines_helper(gpu, prefix):
    """Two frames of 136 x 152 through _twins_encoder against the oracle's encoder in float64: at most 8 times the float32
    oracle encoder's own deviation, in max and mean (fnet: f32 rows; cnet: tanh | relu halves in the engine's activation
    format, which adds the split rows' storage term) - and farther than that from the encoder with blocks.0.1.attn.sr
    transposed (ky <-> kx)."""
    import mof_twins_oracle as to
    from vfml import hip
    from vfml.weights import seeded_state_dict
    cfg, ocfg = _cfgs()
    sd = seeded_state_dict(cfg, 0)
    net = _engine(cfg, sd)
    dev = torch.device("cuda")
    P = net._pack(dev)
    n, H, W = 2, 136, 152
    h, w = H // 8, W // 8
    rows = n * h * w
    x = _frames(n, H, W)[0]
    frames = torch.empty(n * H * W * 4, device="cuda")
    hip.frames_to_nhwc4(x.cuda().contiguous(), n, H, W, 2.0, -1.0, frames)
    out = torch.full((rows * 256,), PATTERN, device="cuda")
    ctx = prefix == "cnet"
    fmt = hip.FMT_S16 if ctx else hip.FMT_F32
    assert net._twins_encoder(prefix, frames, n, H, W, P, dev, out, 256, 0, hip.EPI_TANH_RELU if ctx else hip.EPI_NONE,
                              128 if ctx else 0, out_fmt=fmt) == (h, w)
    torch.cuda.synchronize()
    got = (s16_decode(out, rows, 256, 256) if ctx else out.view(rows, 256).cpu()).double()
    enc = to.TwinsEncoder()
    enc.load_state_dict({k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")})
    enc.eval()

    def run(m, xin):
        with torch.no_grad():
            y = m(2.0 * xin - 1.0)
            if ctx:
                y = torch.cat([torch.tanh(y[:, :128]), torch.relu(y[:, 128:])], dim=1)
        return y.permute(0, 2, 3, 1).reshape(rows, 256).double()
    ref32 = run(enc, x)
    enc = enc.double()
    ref64 = run(enc, x.double())
    with torch.no_grad():
        sr = enc.svt.blocks[0][1].attn.sr
        sr.weight.copy_(sr.weight.transpose(2, 3).clone())
    wrong = run(enc, x.double())
    print(f"[twins {prefix}] mean |map| {ref64.abs().mean().item():.3f}")
    b_max, b_mean = _check(f"twins {prefix}", got, ref64, ref32, fmt)
    d = (got - wrong).abs()
    print(f"[twins {prefix}] from the encoder with sr transposed: max {d.max().item():.3e} mean {d.mean().item():.3e}")
    assert d.max().item() > b_max and d.mean().item() > b_mean


CASES = [(3, 136, 152, {}), (5, 136, 152, {}), (5, 136, 152, {"network": "BOFNet"}), (3, 136, 152, {"sk": True, "gma": True})]


@pytest.mark.parametrize("T,H,W,over", CASES, ids=["mof3", "mof5", "bof5", "twins+sk+gma3"])
def test_twins_forward_matches_oracle(gpu, T, H, W, over):
    """f16x3, depth 4, seed 0, against the float64 oracle: mean EPE <= 8 N, N = the float32 oracle's own mean EPE against
    float64 on that input, and < EPE_TOL; for mof3 all five statistics within 8 times the oracle's noise floor.  All five
    statistics of every one of these cases, of the 1/8-resolution flows, of uint8 input and of flows above one cell are held
    to 8 N by the `twins` cases of tests/test_gpu_elementwise_variants.py."""
    import mof_twins_oracle as to
    from vfml.weights import seeded_state_dict
    cfg, ocfg = _cfgs(**over)
    sd = seeded_state_dict(cfg, 0)
    net = _engine(cfg, sd)
    x = _frames(T, H, W)
    from tests_support import oracle_pair
    pair = oracle_pair(x, ocfg, sd, builder=to)
    ref = pair["f64"][0]
    N = _epe(pair["f32"][0], ref).mean().item()
    got, _ = net(x.cuda(), {})
    got = got.cpu()
    M = 1 if over.get("network") == "BOFNet" else T - 2
    assert got.shape == ref.shape == (1, 2 * M, 2, H, W)
    assert torch.isfinite(got).all()
    e = _epe(got, ref)
    print(f"[twins {over or 'mof'}] T={T} {H}x{W}: mean EPE {e.mean().item():.3e} px, max {e.max().item():.3e} px, N {N:.3e} px, "
          f"mean / N {e.mean().item() / N:.2f}, mean |flow| {ref.abs().mean().item():.3f} px")
    assert e.mean().item() <= K_OF["f16x3"] * N, f"mean EPE {e.mean().item():.3e} px against 8 N = {8 * N:.3e}"
    assert e.mean().item() < EPE_TOL
    if T == 3 and not over:
        assert_within(error_stats(got, ref), noise_floor(x, ocfg, sd, builder=to), 8, "twins mof3")


def test_twins_sliding_job_is_exact(gpu):
    """test_sk_sliding_job_is_exact for a Twins checkpoint at 136 x 152, the prefetch stream left on: all eight fields of an
    8-frame job are bit-identical to the same windows run from scratch with empty caches, and with the graph on to the graph
    off."""
    import numpy as np
    from test_gpu_sk import _sliding_job
    from vfml.synth import synthetic_clip
    from vfml.weights import seeded_state_dict
    cfg, _ = _cfgs()
    sd = seeded_state_dict(cfg, 0)
    clip = torch.from_numpy(np.stack(synthetic_clip(8, 136, 152))).cuda()
    cfg.use_graph = False
    net = _engine(cfg, sd)
    proc, eager = _sliding_job(net, clip)
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
def test_other_checkpoints_pay_nothing(gpu, gma):
    from vfml import build_network, get_cfg
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.decoder_depth, cfg.precision, cfg.gma = DEPTH, "f16x3", gma
    assert cfg.twins is False
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    net.cuda().eval()
    net(_frames(5, 136, 152).cuda(), {})
    assert net.twins is False and not net._twins_spec
    assert not [k for k in net._ws if k.startswith("tw_")]
    assert not [k for k in net._packed if ".svt." in k]
