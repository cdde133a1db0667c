"""The Twins-SVT encoders off the GPU: the parameter table and seeded checkpoints with and without
them, how VideoFlowCore.load_model takes the flag from the checkpoint, the stated limits, the CPU oracle's known answers, the
distance of the definition from its nearest misreadings, and that every parameter tensor reaches the field by more than the
bound the engine is held to (tests/test_gpu_twins.py)."""
import hashlib

import pytest
import torch

from tests_support import K_OF

UB = "update_block"
# SHA-1 of seeded_state_dict(cfg, 0) - keys, shapes and values - computed on the commit BEFORE the Twins encoders were added
PARENT_SHA1 = {
    (False, False): "7c7b4b0ea40e50ad545146908c09821c92a4af17",
    (False, True): "78428fa84573b5815b11219ec09a68454e6459d7",
    (True, False): "aef9fbd6d0a6d1ee46cabe6d18042f579d9d7324",
    (True, True): "35b03486b6f7a0ef9e103cd5e9b580c79a6bd6bb",
}


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


def _table(p):
    """One encoder's parameters, shapes written out: (name, weight shape); every entry has a bias of shape[0] values."""
    sv = f"{p}.svt"
    s = [(f"{sv}.patch_embeds.0.proj", (128, 3, 4, 4)), (f"{sv}.patch_embeds.0.norm", (128,)),
         (f"{sv}.patch_embeds.1.proj", (256, 128, 2, 2)), (f"{sv}.patch_embeds.1.norm", (256,))]
    for i, c, sr in ((0, 128, 8), (1, 256, 4)):
        b = f"{sv}.blocks.{i}.0"
        s += [(f"{b}.norm1", (c,)), (f"{b}.attn.qkv", (3 * c, c)), (f"{b}.attn.proj", (c, c)), (f"{b}.norm2", (c,)),
              (f"{b}.mlp.fc1", (4 * c, c)), (f"{b}.mlp.fc2", (c, 4 * c))]
        b = f"{sv}.blocks.{i}.1"
        s += [(f"{b}.norm1", (c,)), (f"{b}.attn.q", (c, c)), (f"{b}.attn.kv", (2 * c, c)), (f"{b}.attn.proj", (c, c)),
              (f"{b}.attn.sr", (c, c, sr, sr)), (f"{b}.attn.norm", (c,)), (f"{b}.norm2", (c,)), (f"{b}.mlp.fc1", (4 * c, c)),
              (f"{b}.mlp.fc2", (c, 4 * c))]
    s += [(f"{sv}.pos_block.0.proj.0", (128, 1, 3, 3)), (f"{sv}.pos_block.1.proj.0", (256, 1, 3, 3)), (f"{sv}.norm", (1024,))]
    return s


def test_cfg_has_the_flag_off():
    assert _cfg().twins is False


@pytest.mark.parametrize("sk", [False, True])
@pytest.mark.parametrize("gma", [False, True])
def test_twins_table_names_order_and_shapes(sk, gma):
    from vfml import build_network
    from vfml.weights import conv_spec, seeded_state_dict, twins_spec
    import mof_twins_oracle as to
    cfg = _cfg(twins=True, sk=sk, gma=gma)
    table = _table("fnet") + _table("cnet")
    assert [(n, s) for n, _, s in twins_spec(cfg)] == table
    assert not [e for e in conv_spec(cfg) if e[0].startswith(("fnet", "cnet"))]
    assert [e for e in conv_spec(cfg)] == [e for e in conv_spec(_cfg(sk=sk, gma=gma)) if not e[0].startswith(("fnet", "cnet"))]
    sd = seeded_state_dict(cfg, 0)
    keys = list(sd)
    assert keys[:2 * len(table)] == [f"{n}.{p}" for n, _ in table for p in ("weight", "bias")]
    assert keys[2 * len(table)] == (f"{UB}.encoder.convc1.conv_list.0.weight" if sk else f"{UB}.encoder.convc1.weight")
    for n, s in table:
        assert tuple(sd[f"{n}.weight"].shape) == s and tuple(sd[f"{n}.bias"].shape) == s[:1], n
    # LayerNorms are seeded away from (1, 0); a linear weight reaches its bound 1 / sqrt(fan-in)
    for n, s in table:
        if len(s) == 1:
            w, b = sd[f"{n}.weight"], sd[f"{n}.bias"]
            assert 0.75 <= w.min().item() < 0.8 and 1.2 < w.max().item() <= 1.25, n
            assert -0.1 <= b.min().item() < -0.08 and 0.08 < b.max().item() <= 0.1, n
    w = sd["cnet.svt.blocks.1.1.attn.sr.weight"]
    assert 0.99 / 64 < w.abs().max().item() <= 1 / 64
    w = sd["fnet.svt.pos_block.0.proj.0.weight"]
    assert 0.9 / 3 < w.abs().max().item() <= 1 / 3
    # engine and oracle take the same dict, strictly
    net = build_network(cfg)
    net.load_state_dict(sd)
    assert net.twins is True
    ora = to.build_network(_ocfg(twins=True, sk=sk, gma=gma))
    ora.load_state_dict(sd)
    assert sorted(net.state_dict()) == sorted(sd) == sorted(ora.state_dict())
    if not gma:           # (gamma is a parameter of its own module: it sits elsewhere in the module tree's order)
        assert list(net.state_dict()) == keys == list(ora.state_dict())


def _sha1(sd):
    h = hashlib.sha1()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(str(tuple(v.shape)).encode())
        h.update(v.contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("sk,gma", list(PARENT_SHA1))
def test_other_seeded_checkpoints_are_unchanged(sk, gma):
    from vfml.weights import seeded_state_dict
    assert _sha1(seeded_state_dict(_cfg(sk=sk, gma=gma), 0)) == PARENT_SHA1[(sk, gma)]
    assert _sha1(seeded_state_dict(_cfg(sk=sk, gma=gma, twins=False), 0)) == PARENT_SHA1[(sk, gma)]


def _core(tmp_path, monkeypatch, arch="mof"):
    from processing.videoflow_core import VideoFlowCore
    monkeypatch.chdir(tmp_path)
    return VideoFlowCore("cpu", architecture=arch)


def test_load_model_takes_the_flag_from_the_checkpoint(tmp_path, monkeypatch, capsys):
    """The test that fails without the feature: before it, load_checked refused every `fnet.svt.*` checkpoint."""
    from vfml.weights import write_seeded_checkpoint
    write_seeded_checkpoint(str(tmp_path), _cfg(twins=True), seed=1)
    core = _core(tmp_path, monkeypatch)
    core.load_model()
    assert core.cfg.twins is True and core.model.twins is True and core.cfg.sk is False and core.cfg.gma is False
    assert tuple(core.model.state_dict()["cnet.svt.blocks.0.1.attn.sr.weight"].shape) == (128, 128, 8, 8)
    assert not any(k.startswith("fnet.conv1") or ".layer1." in k for k in core.model.state_dict())
    # the released configurations' shape: Twins + SK + GMA, as a BOF checkpoint saved from DataParallel
    write_seeded_checkpoint(str(tmp_path), _cfg(twins=True, sk=True, gma=True), seed=1, architecture="bof", dataparallel_prefix=True)
    core = _core(tmp_path, monkeypatch, arch="bof")
    core.load_model()
    assert core.cfg.twins and core.cfg.sk and core.cfg.gma and core.model.twins and core.model.sk and core.model.gma
    # a plain checkpoint keeps its BasicEncoders
    write_seeded_checkpoint(str(tmp_path), _cfg(), seed=1)
    core = _core(tmp_path, monkeypatch)
    core.load_model()
    assert core.cfg.twins is False and core.model.twins is False
    assert not any(".svt." in k for k in core.model.state_dict())


def test_a_four_stage_backbone_is_refused(tmp_path, monkeypatch, capsys):
    from vfml.weights import checkpoint_name, seeded_state_dict
    sd = seeded_state_dict(_cfg(twins=True), 1)
    for p in ("fnet", "cnet"):
        sd[f"{p}.svt.blocks.2.0.norm1.weight"] = torch.ones(512)
        sd[f"{p}.svt.patch_embeds.2.proj.weight"] = torch.zeros(512, 256, 2, 2)
    (tmp_path / "VideoFlow_ckpt").mkdir()
    torch.save(sd, str(tmp_path / "VideoFlow_ckpt" / checkpoint_name("mof", "sintel", "standard")))
    core = _core(tmp_path, monkeypatch)
    with pytest.raises(RuntimeError, match=r"Twins-SVT \(two stages\) fnet/cnet.*Unexpected key families: cnet\.svt\.\* \(2\), "
                                           r"fnet\.svt\.\* \(2\).*four-stage timm Twins-SVT backbone \(svt\.patch_embeds\.2, "
                                           r"svt\.blocks\.2, \.\.\.\) is the one family that is not supported; Twins-SVT encoders "
                                           r"cut to two stages \(fnet\.svt\.\* / cnet\.svt\.\*\) are, through cfg\.twins"):
        core.load_model()


def test_twins_keys_in_a_plain_network_are_named():
    from vfml import build_network
    from vfml.weights import load_checked, seeded_state_dict
    with pytest.raises(RuntimeError, match=r"CNN BasicEncoder fnet/cnet.*Unexpected key families: cnet\.svt\.\* \(74\), "
                                           r"fnet\.svt\.\* \(74\).*are, through cfg\.twins"):
        load_checked(build_network(_cfg()), seeded_state_dict(_cfg(twins=True), 0), "x.pth")


def test_f32_arithmetic_refuses_a_twins_checkpoint():
    from vfml import build_network
    from vfml.weights import seeded_state_dict
    cfg = _cfg(twins=True, precision="f32")
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    with pytest.raises(ValueError, match="Twins-SVT encoders.*'f32'"):
        net._pack(torch.device("cpu"))


def test_shipped_plans_leave_twins_layers_at_three_terms():
    from vfml import build_network
    from vfml.cfg import BOF_F16_PLAN, DEFAULT_MIXED_PLAN
    from vfml.weights import twins_spec
    for plan in (DEFAULT_MIXED_PLAN, BOF_F16_PLAN):
        net = build_network(_cfg(twins=True, precision="mixed", mfma_plan=plan))
        for name, kind, _ in twins_spec(net.cfg):
            if kind in ("linear", "conv"):
                assert net._nm(name) == 3, name


# ----------------------------------------------------------------------------- known answers of the oracle, float64
def test_layernorm_of_a_constant_row_is_beta():
    import mof_twins_oracle as to
    blk = to.Block(128, 4).double()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        blk.norm1.weight.copy_(torch.rand(128, generator=g, dtype=torch.float64) + 0.5)
        blk.norm1.bias.copy_(torch.randn(128, generator=g, dtype=torch.float64))
        y = blk.norm1(torch.full((3, 5, 128), 2.75, dtype=torch.float64))
    assert (y - blk.norm1.bias).abs().max().item() <= 1e-12
    assert blk.norm1.eps == 1e-5


def test_lsa_with_zero_q_and_k_weights_is_the_window_mean_pad_tokens_included():
    """Scores are then the constant b_q . b_k: every weight 1 / 49.  On a 5 x 9 grid (padded to 7 x 14: two windows) a pad
    token's v is the v bias, and it counts."""
    import mof_twins_oracle as to
    c, heads, h, w = 128, 4, 5, 9
    att = to.LSA(c, heads).double()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, h * w, c, generator=g, dtype=torch.float64)
    with torch.no_grad():
        att.qkv.weight[:2 * c].zero_()
        y = att(x, (h, w))
        v = (x @ att.qkv.weight[2 * c:].T + att.qkv.bias[2 * c:]).view(2, h, w, c)
        vb = att.qkv.bias[2 * c:]
        want = torch.empty(2, h, w, c, dtype=torch.float64)
        want[:, :, :7] = ((v[:, :, :7].sum((1, 2)) + (49 - 35) * vb) / 49)[:, None, None]
        want[:, :, 7:] = ((v[:, :, 7:].sum((1, 2)) + (49 - 10) * vb) / 49)[:, None, None]
        want = att.proj(want.view(2, h * w, c))
    assert (y - want).abs().max().item() <= 1e-12
    assert (want - att.proj.bias).abs().max().item() > 1e-3


def test_gsa_with_zero_q_and_k_weights_is_the_mean_of_the_reduced_tokens():
    import mof_twins_oracle as to
    c, heads, h, w, sr = 128, 4, 17, 19, 8
    att = to.GSA(c, heads, sr).double()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, h * w, c, generator=g, dtype=torch.float64)
    with torch.no_grad():
        att.q.weight.zero_()
        att.kv.weight[:c].zero_()
        y = att(x, (h, w))
        r = att.sr(x.transpose(1, 2).reshape(2, c, h, w))
        assert r.shape == (2, c, 2, 2)                                   # floor(17 / 8) x floor(19 / 8): the rest is dropped
        r = att.norm(r.flatten(2).transpose(1, 2))
        v = r @ att.kv.weight[c:].T + att.kv.bias[c:]
        want = att.proj(v.mean(1, keepdim=True).expand(2, h * w, c))
    assert (y - want).abs().max().item() <= 1e-12


def test_a_zero_depthwise_weight_makes_the_position_block_x_plus_bias():
    import mof_twins_oracle as to
    pos = to.PosConv(128).double()
    x = torch.randn(2, 5 * 9, 128, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    with torch.no_grad():
        pos.proj[0].weight.zero_()
        y = pos(x, (5, 9))
    assert (y - (x + pos.proj[0].bias)).abs().max().item() <= 1e-12


# ----------------------------------------------------------------------------- the definition, pinned by distance
def _frames(T, H, W):
    return torch.rand(1, T, 3, H, W, generator=torch.Generator().manual_seed(T * 1000 + H))


def _epe(a, b):
    return (a.double() - b.double()).pow(2).sum(2).sqrt().mean().item()


_X = {}


def _setup():
    """(seeded dict, frames, float64 field, N) of the committed oracle at T = 3, 136 x 152 (token grids 34 x 38 and 17 x 19,
    both padded in both directions), depth 4, once per session."""
    from vfml.weights import seeded_state_dict
    if not _X:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        sd = seeded_state_dict(_cfg(twins=True), 0)
        x = _frames(3, 136, 152)
        ref = _field(sd, x, torch.float64)
        N = _epe(_field(sd, x, torch.float32), ref)
        print(f"[twins] N = {N:.3e} px, 8 N = {8 * N:.3e} px, mean |flow| {ref.abs().mean().item():.3f} px")
        _X.update(sd=sd, x=x, ref=ref, N=N)
    return _X["sd"], _X["x"], _X["ref"], _X["N"]


def _field(sd, x, dtype=torch.float64):
    import mof_twins_oracle as to
    net = to.build_network(_ocfg(twins=True, decoder_depth=4))
    net.load_state_dict(sd)
    return net.eval().to(dtype)(x.to(dtype), {})[0]


@pytest.mark.parametrize("variant", ["pad_left_top", "mask_pad_keys", "uniform_attention"])
def test_misread_attention_is_far_from_the_definition(variant, monkeypatch):
    """Padding on the left and top, pad keys masked, softmax replaced by uniform weights (the seeded attention is far from
    uniform): each moves the float64 field by more than 8 N."""
    import mof_twins_oracle as to
    sd, x, ref, N = _setup()
    monkeypatch.setitem(to.VARIANT, variant, True)
    S = _epe(_field(sd, x), ref)
    print(f"[twins] {variant}: {S:.3e} px = {S / N:.0f} N")
    assert S > K_OF["f16x3"] * N


@pytest.mark.parametrize("what", ["blocks.0.1.attn.sr", "blocks.1.1.attn.sr", "patch_embeds.0.proj", "patch_embeds.1.proj",
                                  "pos_block.0.proj.0", "pos_block.1.proj.0"])
def test_transposed_kernels_are_far_from_the_definition(what):
    sd, x, ref, N = _setup()
    sd2 = dict(sd)
    for p in ("fnet", "cnet"):
        k = f"{p}.svt.{what}.weight"
        sd2[k] = sd[k].transpose(2, 3).contiguous()
    S = _epe(_field(sd2, x), ref)
    print(f"[twins] {what} transposed (ky <-> kx): {S:.3e} px = {S / N:.0f} N")
    assert S > K_OF["f16x3"] * N


def _slices(sd):
    """(key, row slice or None, inert?) of every tensor of the Twins encoders: qkv cut into q, k, v and kv into k, v; the k
    BIAS slices add the same q . b_k to every score of a query, which softmax does not see."""
    out = []
    for k, v in sd.items():
        if ".svt." not in k or ".svt.norm." in k:
            continue
        name, kind = k.rsplit(".", 1)
        if name.endswith(".attn.qkv") or name.endswith(".attn.kv"):
            c = v.shape[0] // (3 if name.endswith("qkv") else 2)
            for i, part in enumerate("qkv" if name.endswith("qkv") else "kv"):
                out.append((k, slice(i * c, (i + 1) * c), part == "k" and kind == "bias"))
        else:
            out.append((k, None, False))
    return out


def test_every_parameter_tensor_reaches_the_field():
    """Each tensor (slice) replaced by itself plus seeded normal noise of its own mean magnitude - random per element: a
    constant added to a patch-embedding bias is removed by the LayerNorm behind it - moves the float64 field by more than
    8 N; the eight k-bias slices are mathematically inert and move it by less than N; svt.norm is unused."""
    sd, x, ref, N = _setup()
    todo = _slices(sd)
    assert len(todo) == 2 * (72 + 2 * 4 + 2 * 2) and sum(1 for t in todo if t[2]) == 8
    g = torch.Generator().manual_seed(11)
    weakest = None
    for k, sl, inert in todo:
        sd2 = dict(sd)
        t = sd[k].clone()
        part = t if sl is None else t[sl]
        part += torch.randn(part.shape, generator=g) * part.abs().mean()
        sd2[k] = t
        S = _epe(_field(sd2, x), ref)
        tag = k if sl is None else f"{k}[{sl.start}:{sl.stop}]"
        print(f"[twins] {tag}: {S:.3e} px = {S / N:.1f} N{' (inert)' if inert else ''}")
        if inert:
            assert S < N, (tag, S, N)
        else:
            assert S > K_OF["f16x3"] * N, (tag, S, N)
            weakest = (S / N, tag) if weakest is None or S / N < weakest[0] else weakest
    print(f"[twins] weakest: {weakest[1]} at {weakest[0]:.1f} N")
    sd2 = dict(sd)
    for p in ("fnet", "cnet"):
        sd2[f"{p}.svt.norm.weight"] = torch.randn(1024, generator=g)
        sd2[f"{p}.svt.norm.bias"] = torch.randn(1024, generator=g)
    assert torch.equal(_field(sd2, x), ref)
