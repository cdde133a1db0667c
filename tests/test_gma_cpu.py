"""The GMA global-motion aggregator off the GPU: the parameter table and seeded checkpoints with and without it, the CPU
oracle's known answers, and how VideoFlowCore.load_model takes the flag from the checkpoint."""
import math
import os

import pytest
import torch


def _cfg(**over):
    from vfml import get_cfg
    cfg = get_cfg()
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _plain_spec():
    """The parameter table of the network without the aggregator, written out again here."""
    def enc(p):
        s, cin = [(f"{p}.conv1", 64, 3, 7, 7)], 64
        for li, (planes, stride) in enumerate([(64, 1), (96, 2), (128, 2)], start=1):
            for bi in range(2):
                s.append((f"{p}.layer{li}.{bi}.conv1", planes, cin, 3, 3))
                s.append((f"{p}.layer{li}.{bi}.conv2", planes, planes, 3, 3))
                if bi == 0 and stride != 1:
                    s.append((f"{p}.layer{li}.{bi}.downsample.0", planes, cin, 1, 1))
                cin = planes
        return s + [(f"{p}.conv2", 256, 128, 1, 1)]
    ub = "update_block"
    s = enc("fnet") + enc("cnet") + [
        (f"{ub}.encoder.convc1", 256, 648, 1, 1), (f"{ub}.encoder.convc2", 192, 256, 3, 3),
        (f"{ub}.encoder.convf1", 128, 4, 7, 7), (f"{ub}.encoder.convf2", 64, 128, 3, 3),
        (f"{ub}.encoder.conv", 124, 256, 3, 3), (f"{ub}.tprop", 128, 384, 1, 1)]
    s += [(f"{ub}.gru.conv{g}", 128, 512, kh, kw)
          for g, kh, kw in (("z1", 1, 5), ("r1", 1, 5), ("q1", 1, 5), ("z2", 5, 1), ("r2", 5, 1), ("q2", 5, 1))]
    s += [(f"{ub}.flow_head.conv1", 256, 128, 3, 3), (f"{ub}.flow_head.conv2", 4, 256, 3, 3),
          (f"{ub}.mask.0", 256, 128, 3, 3), (f"{ub}.mask.2", 1152, 256, 1, 1)]
    return s


def test_cfg_has_the_flag_off():
    assert _cfg().gma is False


def test_plain_spec_and_seeded_checkpoint_are_unchanged():
    from vfml.weights import conv_spec, seeded_state_dict
    cfg = _cfg()
    assert conv_spec(cfg) == _plain_spec()
    g = torch.Generator().manual_seed(3)
    want = {}
    for name, cout, cin, kh, kw in _plain_spec():
        bound = 1.0 / math.sqrt(cin * kh * kw)
        want[f"{name}.weight"] = (torch.rand(cout, cin, kh, kw, generator=g) * 2 - 1) * bound
        want[f"{name}.bias"] = (torch.rand(cout, generator=g) * 2 - 1) * bound
    got = seeded_state_dict(cfg, 3)
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_gma_spec_keys_and_shapes():
    from vfml.weights import conv_spec, seeded_state_dict
    plain, spec = conv_spec(_cfg()), conv_spec(_cfg(gma=True))
    assert [e[0] for e in spec] == [e[0] for e in plain] + ["att.to_qk", "update_block.aggregator.to_v"]
    assert spec[-2:] == [("att.to_qk", 256, 128, 1, 1), ("update_block.aggregator.to_v", 128, 128, 1, 1)]
    for a, b in zip(plain, spec):
        if ".gru.conv" in a[0]:
            assert b == (a[0], 128, 128 + 4 * 128, a[3], a[4])
        else:
            assert a == b
    sd = seeded_state_dict(_cfg(gma=True), 0)
    psd = seeded_state_dict(_cfg(), 0)
    assert set(sd) - set(psd) == {"att.to_qk.weight", "update_block.aggregator.to_v.weight", "update_block.aggregator.gamma"}
    assert set(psd) <= set(sd)
    assert "att.to_qk.bias" not in sd and "update_block.aggregator.to_v.bias" not in sd
    assert tuple(sd["att.to_qk.weight"].shape) == (256, 128, 1, 1)
    assert tuple(sd["update_block.aggregator.to_v.weight"].shape) == (128, 128, 1, 1)
    assert torch.equal(sd["update_block.aggregator.gamma"], torch.tensor([0.5]))
    assert tuple(sd["update_block.gru.convq2.weight"].shape) == (128, 640, 5, 1)
    # engine and oracle take the same dict, strictly
    from vfml import build_network
    import mof_gma_oracle as go
    build_network(_cfg(gma=True)).load_state_dict(sd)
    go.build_network(_cfg(gma=True)).load_state_dict(sd)
    assert list(build_network(_cfg()).state_dict()) == list(psd)


def _block(gamma, zero_qk):
    import mof_gma_oracle as go
    torch.manual_seed(11)
    att, agg = go.Attention().double(), go.Aggregate().double()
    with torch.no_grad():
        agg.gamma.fill_(gamma)
        if zero_qk:
            att.to_qk.weight.zero_()
    inp = torch.rand(2, 128, 5, 7, dtype=torch.float64)
    mf = torch.randn(2, 128, 5, 7, dtype=torch.float64)
    with torch.no_grad():
        return att, agg, inp, mf, agg(att(inp), mf)


def test_uniform_attention_known_answer():
    """to_qk = 0: every score is zero, attention is uniform, the read-out is the mean of the values over the frame."""
    att, agg, inp, mf, mg = _block(0.5, zero_qk=True)
    with torch.no_grad():
        v = agg.to_v(mf)
    want = mf + 0.5 * v.mean(dim=(2, 3), keepdim=True)
    assert (mg - want).abs().max().item() < 1e-12
    assert (mg - mf).abs().max().item() > 1e-3          # (the block did something)


def test_attention_rows_are_distributions_of_one_frame():
    att, agg, inp, mf, mg = _block(0.5, zero_qk=False)
    with torch.no_grad():
        a = att(inp)
    assert a.shape == (2, 35, 35)
    assert (a.sum(-1) - 1).abs().max().item() < 1e-12
    # frame 1's result does not depend on frame 0's motion features
    mf2 = mf.clone()
    mf2[0] += 1.0
    with torch.no_grad():
        assert torch.equal(agg(a, mf2)[1], mg[1])


def test_gamma_zero_is_the_identity():
    att, agg, inp, mf, mg = _block(0.0, zero_qk=False)
    assert torch.equal(mg, mf)


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
    core = _core(tmp_path, monkeypatch, seeded_state_dict(_cfg(gma=True), 1))
    core.load_model()
    assert core.cfg.gma is True and core.model.gma is True
    assert core.model.state_dict()["update_block.aggregator.gamma"].item() == 0.5
    info = core.get_model_info()
    assert set(info["config"]) == {"decoder_depth", "corr_levels", "corr_radius"}
    core = _core(tmp_path, monkeypatch, {"module." + k: v for k, v in seeded_state_dict(_cfg(), 1).items()}, arch="bof")
    core.load_model()
    assert core.cfg.gma is False and core.model.gma is False
    assert not any("aggregator" in k or k.startswith("att.") for k in core.model.state_dict())


def test_gma_checkpoint_with_wrong_gate_shapes_is_refused(tmp_path, monkeypatch, capsys):
    from vfml.weights import seeded_state_dict
    sd = seeded_state_dict(_cfg(gma=True), 1)
    plain = seeded_state_dict(_cfg(), 1)
    for k in plain:
        if ".gru.conv" in k:
            sd[k] = plain[k]          # gates of the network without the fourth input block
    core = _core(tmp_path, monkeypatch, sd)
    with pytest.raises(RuntimeError, match="parameter shapes differ.*update_block.gru.convz1.weight"):
        core.load_model()


def test_aggregator_keys_without_gamma_are_named(tmp_path, monkeypatch, capsys):
    """A checkpoint with aggregator convolutions but no gamma builds the plain network; the refusal names the families and
    says that the aggregator itself is supported."""
    from vfml.weights import seeded_state_dict
    sd = seeded_state_dict(_cfg(gma=True), 1)
    del sd["update_block.aggregator.gamma"]
    core = _core(tmp_path, monkeypatch, sd)
    with pytest.raises(RuntimeError, match=r"att\.to_qk.*GMA aggregator .* is, through cfg.gma"):
        core.load_model()


def test_f32_arithmetic_refuses_a_gma_checkpoint():
    """The aggregator is built on the split-f16 kernels only: the exact-f32 arithmetic says so when the weights are packed,
    and still runs a plain checkpoint's packing."""
    from vfml import build_network
    from vfml.weights import seeded_state_dict
    cfg = _cfg(gma=True, precision="f32")
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    with pytest.raises(ValueError, match="GMA aggregator.*'f32'"):
        net._pack(torch.device("cpu"))
    cfg = _cfg(precision="f32")
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    assert "update_block.gru.convq2.iter" in net._pack(torch.device("cpu"))


def test_attention_form_by_frame_size():
    """Which frames keep their attention as the f16 plane and which as split rows (MemFlow's conditions)."""
    from vfml.network import MOFNetHIP
    assert MOFNetHIP._attention_geometry(32400) == (32400, 32448, True)       # 1080p: the plain-f16 plane
    assert MOFNetHIP._attention_geometry(1056) == (1056, 1088, True)
    assert MOFNetHIP._attention_geometry(323) == (328, 384, False)            # small: split rows
    assert MOFNetHIP._attention_geometry(1023)[2] is False
