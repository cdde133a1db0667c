"""The SK update block off the GPU: the parameter table and seeded checkpoints with and without it, the CPU oracle's known
answers, how VideoFlowCore.load_model takes the flag from the checkpoint, the stated limits, and that every depthwise
convolution of the block reaches the field by more than the bound the engine is held to (tests/test_gpu_sk.py)."""
import math

import pytest
import torch

from tests_support import K_OF

UB = "update_block"


def _cfg(**over):
    from vfml import get_cfg
    cfg = get_cfg()
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _ocfg(**over):
    from oracle import mof_oracle as mo
    cfg = mo.get_cfg()
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _enc(p):
    s, cin = [(f"{p}.conv1", 64, 3, 7, 7)], 64
    for li, (planes, stride) in enumerate([(64, 1), (96, 2), (128, 2)], start=1):
        for bi in range(2):
            s.append((f"{p}.layer{li}.{bi}.conv1", planes, cin, 3, 3))
            s.append((f"{p}.layer{li}.{bi}.conv2", planes, planes, 3, 3))
            if bi == 0 and stride != 1:
                s.append((f"{p}.layer{li}.{bi}.downsample.0", planes, cin, 1, 1))
            cin = planes
    return s + [(f"{p}.conv2", 256, 128, 1, 1)]


def _pc(name, c, hid, cout, k1):
    """A PCBlock's seven entries, shapes written out (hid given, not computed)."""
    return [(f"{name}.conv_list.0", c, 1, 1, 1), (f"{name}.conv_list.1", c, 1, k1, k1),
            (f"{name}.ffn1.0", hid, c, 1, 1), (f"{name}.ffn1.2", c, hid, 1, 1), (f"{name}.pw", c, c, 1, 1),
            (f"{name}.ffn2.0", hid, c, 1, 1), (f"{name}.ffn2.2", cout, hid, 1, 1)]


def _sk_spec(gma):
    """The SK parameter table, written out again here."""
    s = _enc("fnet") + _enc("cnet")
    s += _pc(f"{UB}.encoder.convc1", 648, 972, 256, 15) + _pc(f"{UB}.encoder.convc2", 256, 384, 192, 15)
    s += [(f"{UB}.encoder.convf1", 128, 4, 1, 1)]
    s += _pc(f"{UB}.encoder.convf2", 128, 192, 64, 15) + _pc(f"{UB}.encoder.conv", 256, 384, 124, 15)
    s += [(f"{UB}.tprop", 128, 384, 1, 1)]
    s += _pc(f"{UB}.gru", 640, 960, 128, 7) if gma else _pc(f"{UB}.gru", 512, 768, 128, 7)
    s += _pc(f"{UB}.flow_head", 128, 192, 4, 15)
    s += [(f"{UB}.mask.0", 256, 128, 3, 3), (f"{UB}.mask.2", 1152, 256, 1, 1)]
    if gma:
        s += [("att.to_qk", 256, 128, 1, 1), (f"{UB}.aggregator.to_v", 128, 128, 1, 1)]
    return s


def test_cfg_has_the_flag_off():
    assert _cfg().sk is False


@pytest.mark.parametrize("gma", [False, True])
def test_sk_spec_names_order_and_shapes(gma):
    from vfml.weights import conv_spec, seeded_state_dict
    cfg = _cfg(sk=True, gma=gma)
    assert conv_spec(cfg) == _sk_spec(gma)
    sd = seeded_state_dict(cfg, 0)
    assert tuple(sd[f"{UB}.gru.ffn1.0.weight"].shape) == ((960, 640, 1, 1) if gma else (768, 512, 1, 1))
    assert tuple(sd[f"{UB}.encoder.convc1.conv_list.1.weight"].shape) == (648, 1, 15, 15)
    assert tuple(sd[f"{UB}.gru.conv_list.1.weight"].shape) == (640 if gma else 512, 1, 7, 7)
    # key order: per block conv_list.0, conv_list.1, ffn1.0, ffn1.2, pw, ffn2.0, ffn2.2 (weight, bias each)
    keys = [k for k in sd if k.startswith(f"{UB}.flow_head.")]
    assert keys == [f"{UB}.flow_head.{n}.{p}" for n in ("conv_list.0", "conv_list.1", "ffn1.0", "ffn1.2", "pw", "ffn2.0", "ffn2.2")
                    for p in ("weight", "bias")]
    # a depthwise weight is drawn with bound 1 / k (fan-in k * k), and reaches it
    w = sd[f"{UB}.flow_head.conv_list.1.weight"]
    assert w.abs().max().item() <= 1 / 15 and w.abs().max().item() > 0.9 / 15
    assert (f"{UB}.aggregator.gamma" in sd) == gma
    # engine and oracle take the same dict, strictly
    from vfml import build_network
    import mof_sk_oracle as so
    build_network(cfg).load_state_dict(sd)
    so.build_network(_ocfg(sk=True, gma=gma)).load_state_dict(sd)
    keys = list(build_network(cfg).state_dict())
    assert sorted(keys) == sorted(sd)
    if not gma:           # (gamma is a parameter of its own module: it sits elsewhere in the module tree's order)
        assert keys == list(sd)


def test_plain_and_gma_tables_are_unchanged():
    from vfml.weights import conv_spec, seeded_state_dict
    plain = _enc("fnet") + _enc("cnet") + [
        (f"{UB}.encoder.convc1", 256, 648, 1, 1), (f"{UB}.encoder.convc2", 192, 256, 3, 3),
        (f"{UB}.encoder.convf1", 128, 4, 7, 7), (f"{UB}.encoder.convf2", 64, 128, 3, 3),
        (f"{UB}.encoder.conv", 124, 256, 3, 3), (f"{UB}.tprop", 128, 384, 1, 1)]
    plain += [(f"{UB}.gru.conv{g}", 128, 512, kh, kw)
              for g, kh, kw in (("z1", 1, 5), ("r1", 1, 5), ("q1", 1, 5), ("z2", 5, 1), ("r2", 5, 1), ("q2", 5, 1))]
    plain += [(f"{UB}.flow_head.conv1", 256, 128, 3, 3), (f"{UB}.flow_head.conv2", 4, 256, 3, 3),
              (f"{UB}.mask.0", 256, 128, 3, 3), (f"{UB}.mask.2", 1152, 256, 1, 1)]
    assert conv_spec(_cfg()) == plain == conv_spec(_cfg(sk=False))
    gma = conv_spec(_cfg(gma=True))
    assert [e[0] for e in gma] == [e[0] for e in plain] + ["att.to_qk", f"{UB}.aggregator.to_v"]
    g = torch.Generator().manual_seed(5)
    sd = seeded_state_dict(_cfg(), 5)
    for name, cout, cin, kh, kw in plain:
        bound = 1.0 / math.sqrt(cin * kh * kw)
        assert torch.equal(sd[f"{name}.weight"], (torch.rand(cout, cin, kh, kw, generator=g) * 2 - 1) * bound), name
        assert torch.equal(sd[f"{name}.bias"], (torch.rand(cout, generator=g) * 2 - 1) * bound), name
    assert not any(".conv_list." in k or ".ffn1." in k for k in sd)


def _core(tmp_path, monkeypatch, sd, arch="mof"):
    from processing.videoflow_core import VideoFlowCore
    from vfml.weights import checkpoint_name
    d = tmp_path / "VideoFlow_ckpt"
    d.mkdir(exist_ok=True)
    torch.save(sd, str(d / checkpoint_name(arch, "sintel", "standard")))
    monkeypatch.chdir(tmp_path)
    return VideoFlowCore("cpu", architecture=arch)


def test_load_model_takes_the_flag_from_the_checkpoint(tmp_path, monkeypatch, capsys):
    from vfml.weights import seeded_state_dict
    core = _core(tmp_path, monkeypatch, seeded_state_dict(_cfg(sk=True), 1))
    core.load_model()
    assert core.cfg.sk is True and core.model.sk is True and core.cfg.gma is False
    assert tuple(core.model.state_dict()[f"{UB}.gru.conv_list.1.weight"].shape) == (512, 1, 7, 7)
    assert set(core.get_model_info()["config"]) == {"decoder_depth", "corr_levels", "corr_radius"}
    core = _core(tmp_path, monkeypatch, seeded_state_dict(_cfg(sk=True, gma=True), 1))
    core.load_model()
    assert core.cfg.sk is True and core.cfg.gma is True and core.model.sk and core.model.gma
    core = _core(tmp_path, monkeypatch, {"module." + k: v for k, v in seeded_state_dict(_cfg(), 1).items()}, arch="bof")
    core.load_model()
    assert core.cfg.sk is False and core.model.sk is False
    assert not any(".conv_list." in k for k in core.model.state_dict())


def test_sk_checkpoint_with_gamma_but_narrow_gru_is_refused(tmp_path, monkeypatch, capsys):
    from vfml.weights import seeded_state_dict
    sd = seeded_state_dict(_cfg(sk=True), 1)            # gru over 512 channels
    for k, v in seeded_state_dict(_cfg(sk=True, gma=True), 1).items():
        if k.startswith("att.") or ".aggregator." in k:
            sd[k] = v
    core = _core(tmp_path, monkeypatch, sd)
    with pytest.raises(RuntimeError, match=r"parameter shapes differ.*update_block\.gru\.conv_list\.0\.weight: checkpoint "
                                           r"\(512, 1, 1, 1\) vs network \(640, 1, 1, 1\)"):
        core.load_model()


def test_sk_keys_in_a_plain_network_are_named():
    """load_checked names the SK block as supported through cfg.sk and the Twins-SVT encoders as the one missing family."""
    from vfml import build_network
    from vfml.weights import load_checked, seeded_state_dict
    with pytest.raises(RuntimeError, match=r"update_block\.encoder\.\*.*Twins-SVT.*one family that is not supported.*"
                                           r"SK update block .* is, through cfg.sk"):
        load_checked(build_network(_cfg()), seeded_state_dict(_cfg(sk=True), 0), "x.pth")


def test_fast_lookup_is_refused_by_engine_and_oracle():
    from vfml import build_network
    import mof_sk_oracle as so
    with pytest.raises(ValueError, match=r"SK update block needs the base lookup .*\(4, 4\), got \(2, 3\)"):
        build_network(_cfg(sk=True, corr_levels=2, corr_radius=3))
    with pytest.raises(ValueError, match=r"SK update block needs the base lookup .*\(4, 4\), got \(2, 3\)"):
        so.build_network(_ocfg(sk=True, corr_levels=2, corr_radius=3))
    build_network(_cfg(corr_levels=2, corr_radius=3))          # (a plain checkpoint keeps --fast)


def test_f32_arithmetic_refuses_an_sk_checkpoint():
    from vfml import build_network
    from vfml.weights import seeded_state_dict
    cfg = _cfg(sk=True, precision="f32")
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    with pytest.raises(ValueError, match="SK update block.*'f32'"):
        net._pack(torch.device("cpu"))


def test_shipped_plans_do_not_reach_sk_layers():
    """Plan entries are name prefixes; the plain block's layer names prefix the PCBlocks' (`...encoder.convc1` and
    `...encoder.convc1.ffn1.0`).  Under cfg.sk only the "" default of a plan applies to a PCBlock's layers."""
    from vfml import build_network
    from vfml.cfg import BOF_F16_PLAN, DEFAULT_MIXED_PLAN
    net = build_network(_cfg(sk=True, precision="mixed", mfma_plan=DEFAULT_MIXED_PLAN))
    sk_layers = [n for b in net._sk_blocks for n in (f"{b}.ffn1.0", f"{b}.ffn1.2", f"{b}.pw", f"{b}.ffn2.0", f"{b}.ffn2.2")]
    sk_layers.append(f"{UB}.encoder.convf1")
    assert len(sk_layers) == 31
    for n in sk_layers:
        assert net._nm(n) == 3, n
    assert net._nm(f"{UB}.mask.0") == 1 and net._nm(f"{UB}.tprop") == "2a"       # (layers the two blocks share)
    net = build_network(_cfg(sk=True, precision="mixed", mfma_plan=BOF_F16_PLAN))
    for n in sk_layers:
        assert net._nm(n) == 1, n
    net = build_network(_cfg(sk=True, precision="mixed", mfma_plan={f"{UB}.gru.": 2, f"{UB}.gru.pw": 1}))
    assert net._nm(f"{UB}.gru.ffn1.0") == 2 and net._nm(f"{UB}.gru.pw") == 1 and net._nm(f"{UB}.flow_head.pw") == 3


# ----------------------------------------------------------------------------- known answers of the oracle, float64
def test_gelu_is_the_erf_form():
    import mof_sk_oracle as so
    blk = so.PCBlock(8, 8, (1, 3)).double()
    one = torch.ones(1, dtype=torch.float64)
    assert abs(blk.ffn1[1](one).item() - 0.8413447460685429) < 1e-15
    assert abs(torch.nn.functional.gelu(one, approximate="tanh").item() - 0.8413447460685429) > 1e-4


def test_zero_block_returns_its_last_bias():
    import mof_sk_oracle as so
    blk = so.PCBlock(16, 4, (1, 15)).double()
    with torch.no_grad():
        for p in blk.parameters():
            p.zero_()
        blk.ffn2[2].bias.copy_(torch.tensor([1.5, -2.0, 0.25, 3.0], dtype=torch.float64))
        y = blk(torch.randn(2, 16, 9, 11, dtype=torch.float64))
    assert y.shape == (2, 4, 9, 11)
    assert torch.equal(y, torch.tensor([1.5, -2.0, 0.25, 3.0], dtype=torch.float64).view(1, 4, 1, 1).expand(2, 4, 9, 11))


def test_single_tap_pins_orientation_and_padding():
    """A 15 x 15 depthwise weight with one tap of value 1 at (ky, kx) = (7 + 3, 7 - 5): conv[y][x] = in[y + 3][x - 5], zeros
    outside the frame - on a 9 x 11 frame, smaller than the kernel."""
    import mof_sk_oracle as so
    blk = so.PCBlock(4, 4, (1, 15)).double()
    conv = blk.conv_list[1]
    with torch.no_grad():
        conv.weight.zero_()
        conv.bias.zero_()
        conv.weight[:, 0, 7 + 3, 7 - 5] = 1.0
        x = torch.randn(1, 4, 9, 11, dtype=torch.float64)
        y = conv(x)
    want = torch.zeros_like(x)
    want[:, :, 0:6, 5:11] = x[:, :, 3:9, 0:6]
    assert torch.equal(y, want)


# ----------------------------------------------------------------------------- every depthwise convolution reaches the field
SEED = 0        # the first seed in 0..7 whose twelve S exceed 8 N (module docstring of tests/test_gpu_sk.py takes it from here)


def _frames(T, H, W):
    return torch.rand(1, T, 3, H, W, generator=torch.Generator().manual_seed(T * 1000 + H))


def _epe(a, b):
    return (a.double() - b.double()).pow(2).sum(2).sqrt().mean().item()


def test_every_depthwise_convolution_reaches_the_field():
    """T = 3, 136 x 152, depth 4: the float32 oracle with one `conv_list` weight zeroed differs from the intact one by a mean
    EPE S; S > 8 N for all twelve, N = the float32 oracle's mean EPE against the float64 one on that input.  This involves
    the oracle alone; it is what lets the end-to-end bound of tests/test_gpu_sk.py (mean EPE <= 8 N) see a skipped
    convolution."""
    import mof_sk_oracle as so
    from vfml.weights import seeded_state_dict
    sd = seeded_state_dict(_cfg(sk=True), SEED)
    x = _frames(3, 136, 152)

    def field(state, dtype):
        net = so.build_network(_ocfg(sk=True, decoder_depth=4))
        net.load_state_dict(state)
        net = net.eval().to(dtype)
        return net(x.to(dtype), {})[0]

    ref32 = field(sd, torch.float32)
    N = _epe(ref32, field(sd, torch.float64))
    assert torch.isfinite(ref32).all()
    print(f"[sk] seed {SEED}: N = {N:.3e} px, bound 8 N = {K_OF['f16x3'] * N:.3e} px, mean |flow| {ref32.abs().mean().item():.3f} px")
    names = [k for k in sd if ".conv_list." in k and k.endswith(".weight")]
    assert len(names) == 12
    worst = None
    for k in names:
        sd0 = dict(sd)
        sd0[k] = torch.zeros_like(sd[k])
        S = _epe(field(sd0, torch.float32), ref32)
        print(f"[sk] {k}: S = {S:.3e} px")
        worst = S if worst is None else min(worst, S)
        assert S > K_OF["f16x3"] * N, (k, S, N)
