"""Stage parity of the encoders: MOFNetHIP._encoder against oracle.fnet / oracle.cnet in float64.

The end-to-end tests see the encoders through a whole field; here their output is compared directly, at shapes chosen so
that every dispatch branch of `conv_stats` is taken (fused statistics partials or the separate statistics pass, the
64-channel layer1 kernel or the general one, the stem kernel, ragged last statistics blocks) - which
test_encoder_cases_reach_every_branch proves with counting spies - and on inputs whose activations are degenerate (all-black,
all-white, flat frames: a layer that is constant away from the border has almost no variance).

Statistics: max |error| over max |reference|; and, per channel, max |error| over that channel's rms, the worst channel
(a wrong norm statistic of one channel shows here, not in the first).  The rms is that of the channel as the last
convolution leaves it in the float64 oracle, before cnet's tanh / relu: both are 1-Lipschitz, so that is the scale of the
channel's error, whereas a context channel that relu leaves almost everywhere at zero has an rms of its own that says
nothing about it.  (With the rms of the activated channel, floored at 1e-3 of the map's, the statistic of the float32
oracle itself spread from 9e-5 to 2e-3 over the inputs and the exact-f32 engine measured 0.5 to 6.3 times it, worst on the
near-dead channels, while fnet - no activation - stayed between 1.0 and 2.1 times: that was the denominator, not the engine.)
Bound: K (4 for f32, 8 for f16x3: tests_support.K_OF) times the same statistic of the float32 oracle encoder against the
float64 one on the same frames."""
import pytest
import torch

import tests_support as ts

pytestmark = pytest.mark.gpu

# (n, H, W).  (3,128,128): everything fused, layer1 through the 64-channel kernel.  (4,136,160) / (1,136,160): layer2 has 1360
# and layer3 340 pixels per image, no multiples of 32: n = 4 takes the separate statistics pass, n = 1 a ragged last block;
# W/2 = 80 keeps the 64-channel kernel out.  (2,64,200): layer3 has 200 pixels.  1080 x 1920 (layer3: 32400 pixels, ragged),
# 1088 x 1920 (everything whole) and 880 x 1280 (a 4K tile): full sizes, one frame.
SMALL_SHAPES = [(3, 128, 128), (4, 136, 160), (1, 136, 160), (2, 64, 200)]
BIG_SHAPES = [(1, 1080, 1920), (1, 1088, 1920), (1, 880, 1280)]
CASES = ([(kind,) + s for s in SMALL_SHAPES for kind in ts.INPUT_KINDS] +
         [("clip",) + s for s in BIG_SHAPES] + [("black", 1, 1080, 1920)])
SPIED = ("conv3x3_c64", "stem7x7s2", "instnorm_stats", "instnorm_finalize")

_REF = {}


def _state():
    from vfml import get_cfg
    from vfml.weights import seeded_state_dict
    return seeded_state_dict(get_cfg(), 0)


def _oracle_maps(kind, n, H, W, prefix):
    """(float32 oracle map, float64 oracle map, rms per channel of the float64 map before cnet's activation) of encoder
    `prefix`, maps [n, 256, H/8, W/8], once per session."""
    key = (kind, n, H, W, prefix)
    if key not in _REF:
        sd = _state()
        cfg = ts.oracle_cfg()
        x = ts.to_float_frames(ts.make_frames(kind, n, H, W))[0]
        out = []
        with torch.no_grad():
            for ora, xin in ((ts.oracle_f32(cfg, sd), x), (ts.oracle_f64(cfg, sd), x.double())):
                y = getattr(ora, prefix)(cfg.input_scale * xin + cfg.input_shift)
                rms = y.pow(2).mean(dim=(0, 2, 3)).sqrt()
                if prefix == "cnet":
                    y = torch.cat([torch.tanh(y[:, :128]), torch.relu(y[:, 128:])], dim=1)
                out.append(y)
        _REF[key] = tuple(out) + (rms,)
    return _REF[key]


def _engine(precision):
    from vfml import build_network, get_cfg
    cfg = get_cfg()
    cfg.precision = precision
    net = build_network(cfg)
    net.load_state_dict(_state())
    return net.cuda().eval()


def _encode(net, prefix, u8):
    """u8 [n, H, W, 3] device frames through K1 and MOFNetHIP._encoder -> [n, 256, H/8, W/8] on the host."""
    from vfml import hip
    n, H, W, _ = u8.shape
    dev = u8.device
    with torch.cuda.device(dev):
        P = net._pack(dev)
        frames = torch.empty(n * H * W * 4, device=dev)
        hip.frames_to_nhwc4(u8.contiguous(), n, H, W, float(net.cfg.input_scale), float(net.cfg.input_shift), frames)
        out = torch.full((n * (H // 8) * (W // 8) * 256,), float("nan"), device=dev)
        epi, split = (hip.EPI_NONE, 0) if prefix == "fnet" else (hip.EPI_TANH_RELU, 128)
        hh, ww = net._encoder(prefix, frames, n, H, W, P, dev, out, 256, 0, epi, split)
    assert (hh, ww) == (H // 8, W // 8)
    return out.view(n, hh, ww, 256).permute(0, 3, 1, 2).cpu()


def _stage_stats(got, ref, rms_c):
    err = (got.double() - ref).abs()
    return {"overall": float(err.max() / ref.abs().max()), "channel": float((err.amax(dim=(0, 2, 3)) / rms_c).max())}


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("prefix", ["fnet", "cnet"])
@pytest.mark.parametrize("kind,n,H,W", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in CASES])
def test_encoder_output_within_k_times_the_oracles_own_noise(gpu, kind, n, H, W, prefix, precision):
    o32, o64, rms = _oracle_maps(kind, n, H, W, prefix)
    N = _stage_stats(o32, o64, rms)
    u8 = ts.make_frames(kind, n, H, W).cuda()
    net = _engine(precision)
    try:
        got = _encode(net, prefix, u8)
        alone = [_encode(net, prefix, u8[i:i + 1]) for i in range(n)] if n > 1 else []
    finally:
        net.release_workspace()
        del net
        torch.cuda.empty_cache()
    assert torch.isfinite(got).all()
    E = _stage_stats(got, o64, rms)
    K = ts.K_OF[precision]
    print(f"STAGE|{prefix}|{kind}|{n}x{H}x{W}|{precision}|N overall {N['overall']:.2e} channel {N['channel']:.2e}|"
          f"engine overall {E['overall']:.2e} channel {E['channel']:.2e}|ratio {E['overall'] / N['overall']:.2f} "
          f"{E['channel'] / N['channel']:.2f}")
    for k in ("overall", "channel"):
        assert E[k] <= K * N[k], f"{k}: engine {E[k]:.3e} > {K:g} x N = {K * N[k]:.3e}"
    # a frame's maps do not depend on what it is batched with (the sliding-window cache encodes a new frame alone)
    for i, a in enumerate(alone):
        assert torch.equal(a[0], got[i]), f"frame {i} of the batch differs from the frame encoded alone: " \
            f"{int((a[0] != got[i]).sum())} values, max {float((a[0] - got[i]).abs().max()):.3g}"


def test_encoder_cases_reach_every_branch(gpu, monkeypatch):
    """The shapes above, run with counting spies on the kernels `conv_stats` chooses between: each is reached with one
    frame and with several; in the split arithmetic the separate statistics pass is the several-frames fallback only, one
    frame meets a ragged last statistics block, and layer1 runs with and without the 64-channel kernel."""
    from vfml import hip
    calls = []          # (kernel, precision, n, hw of an instnorm_finalize or None)
    state = {}
    for name in SPIED:
        real = getattr(hip, name)

        def spy(*a, _real=real, _name=name, **kw):
            hw = a[4] if _name == "instnorm_finalize" else None
            calls.append((_name, state["precision"], state["n"], hw))
            return _real(*a, **kw)
        monkeypatch.setattr(hip, name, spy)
    shapes = sorted(set(c[1:] for c in CASES))
    with_c64 = {}
    for precision in ("f32", "f16x3"):
        net = _engine(precision)
        for n, H, W in shapes:
            state.update(precision=precision, n=n)
            before = len(calls)
            _encode(net, "fnet", ts.make_frames("rand", n, H, W).cuda())
            with_c64[(precision, n, H, W)] = any(c[0] == "conv3x3_c64" for c in calls[before:])
        net.release_workspace()
        del net
        torch.cuda.empty_cache()
    for name in SPIED:
        assert any(c[0] == name and c[2] == 1 for c in calls), f"{name} never reached with one frame"
        assert any(c[0] == name and c[2] > 1 for c in calls), f"{name} never reached with several frames"
    split = [c for c in calls if c[1] == "f16x3"]
    assert any(c[0] == "instnorm_stats" and c[2] > 1 for c in split)            # hw % 32 != 0 with several frames
    assert not any(c[0] == "instnorm_stats" and c[2] == 1 for c in split)       # one frame: always the fused partials
    assert any(c[0] == "instnorm_finalize" and c[2] == 1 and c[3] % hip.STATS_ROWS_S16 for c in split)   # ragged last block
    assert any(c[0] == "instnorm_finalize" and c[2] > 1 for c in split)
    for many in (False, True):
        took = {v for (p, n, H, W), v in with_c64.items() if p == "f16x3" and (n > 1) == many}
        assert took == {True, False}, (many, took)
    assert not any(c[0] in ("conv3x3_c64", "stem7x7s2", "instnorm_finalize") for c in calls if c[1] == "f32")
    print("encoder kernels reached:", {(k, p, "n=1" if n == 1 else "n>1"): sum(1 for c in calls if c[0] == k and c[1] == p and (c[2] == 1) == (n == 1))
                                      for k in SPIED for p in ("f32", "f16x3") for n in (1, 2)})
