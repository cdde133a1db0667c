"""The GMA global-motion aggregator on the GPU: the engine with a seeded GMA checkpoint against the CPU oracle of
tests/mof_gma_oracle.py, its caches and graphs in a sliding job, and that a plain checkpoint pays nothing for it."""
import pytest
import torch

from tests_support import EPE_TOL

pytestmark = pytest.mark.gpu

DEPTH = 4


def _cfgs(**over):
    from oracle import mof_oracle as mo
    from vfml import get_cfg
    cfg, ocfg = get_cfg(), mo.get_cfg()
    for c in (cfg, ocfg):
        c.gma, c.decoder_depth = True, DEPTH
        for k, v in over.items():
            setattr(c, k, v)
    cfg.precision = "f16x3"
    return cfg, ocfg


def _engine(cfg, sd):
    from vfml import build_network
    net = build_network(cfg)
    net.load_state_dict(sd)
    return net.cuda().eval()


def _pair(seed=0, **over):
    import mof_gma_oracle as go
    from vfml.weights import seeded_state_dict
    cfg, ocfg = _cfgs(**over)
    sd = seeded_state_dict(cfg, seed)
    ora = go.build_network(ocfg)
    ora.load_state_dict(sd)
    return _engine(cfg, sd), ora.eval(), sd


def _epe(a, b):
    return (a - b).pow(2).sum(2).sqrt()


def _frames(T, H, W):
    return torch.rand(1, T, 3, H, W, generator=torch.Generator().manual_seed(T * 1000 + H))


_REF = {}


def _oracle_field(T, H, W, network="MOFNetStack"):
    """The oracle's field for _frames(T, H, W), once per session."""
    key = (T, H, W, network)
    if key not in _REF:
        _, ora, _ = _pair(network=network)
        _REF[key] = ora(_frames(T, H, W), {})[0]
    return _REF[key]


@pytest.mark.parametrize("T,H,W,form", [(5, 256, 264, "plane"), (3, 136, 152, "rows"), (5, 136, 152, "rows")])
def test_gma_forward_matches_oracle(gpu, T, H, W, form):
    """32 x 33 cells (P = 1056) takes the resident f16 plane, 17 x 19 (P = 323) the split-row probabilities.  A bound on the
    mean alone: the same fields are held to the float64 oracle statistic by statistic, with the 1/8-resolution flows, in
    tests/test_gpu_elementwise_variants.py."""
    net, _, _ = _pair()
    ref = _oracle_field(T, H, W)
    got, _ = net(_frames(T, H, W).cuda(), {})
    got = got.cpu()
    assert net._att_store.plain == (form == "plane")
    assert got.shape == ref.shape == (1, 2 * (T - 2), 2, H, W)
    assert torch.isfinite(got).all()
    e = _epe(got, ref)
    print(f"[gma {form}] T={T} {H}x{W}: mean EPE {e.mean().item():.3e} px, max {e.max().item():.3e} px, "
          f"mean |flow| {ref.abs().mean().item():.3f} px")
    assert e.mean().item() < EPE_TOL, f"mean EPE {e.mean().item():.3e} px (max {e.max().item():.3e})"


def test_gma_bof_matches_oracle(gpu):
    T, H, W = 5, 256, 264
    net, _, _ = _pair(network="BOFNet")
    ref = _oracle_field(T, H, W, "BOFNet")
    got, _ = net(_frames(T, H, W).cuda(), {})
    got = got.cpu()
    assert got.shape == ref.shape == (1, 2, 2, H, W)
    e = _epe(got, ref)
    print(f"[gma bof] T={T} {H}x{W}: mean EPE {e.mean().item():.3e} px, max {e.max().item():.3e} px, "
          f"mean |flow| {ref.abs().mean().item():.3f} px")
    assert e.mean().item() < EPE_TOL, f"mean EPE {e.mean().item():.3e} px (max {e.max().item():.3e})"


def test_gamma_reaches_the_field(gpu):
    """The same weights with gamma = 0 and gamma = 0.5 give fields further apart than the tolerance the engine is held to:
    an aggregator that is silently skipped cannot pass the oracle test."""
    from vfml.weights import seeded_state_dict
    cfg, _ = _cfgs()
    sd = seeded_state_dict(cfg, 0)
    x = _frames(5, 256, 264).cuda()
    a = _engine(cfg, sd)(x, {})[0].clone()
    sd0 = dict(sd)
    sd0["update_block.aggregator.gamma"] = torch.zeros(1)
    b = _engine(cfg, sd0)(x, {})[0]
    d = _epe(a, b).mean().item()
    print(f"[gma] gamma 0.5 against gamma 0: mean EPE {d:.3e} px")
    assert d > EPE_TOL


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


def test_gma_sliding_job_is_exact(gpu):
    """Planes kept per frame and reused by overlapping windows, the prefetch side stream, the iteration-zero store, pick_only
    and the replayed graph: every field of an 8-frame job is bit-identical to the same window run from scratch with empty
    caches (unkeyed, all centres, the whole output), and with the graph on to the graph off.  Four of the eight windows
    are clamped at an end of the clip and hold one frame several times: those are the ones in which a frame's plane and
    slots are reused within a window, and the ones that need a frame's forward and backward volume against itself kept
    apart (network.py _window_pyramids)."""
    import numpy as np
    from vfml.synth import synthetic_clip
    from vfml.weights import seeded_state_dict
    cfg, _ = _cfgs()
    sd = seeded_state_dict(cfg, 0)
    clip = torch.from_numpy(np.stack(synthetic_clip(8, 256, 264))).cuda()
    cfg.use_graph = False
    net = _engine(cfg, sd)
    proc, eager = _sliding_job(net, clip)
    assert net.iter0_stats["warm"] > 0
    clamped = 0
    for i in range(8):
        idx = list(proc.window_indices(8, i))
        clamped += len(set(idx)) < len(idx)
        net.clear_feature_cache()
        b, _ = net.forward_u8(clip[idx])
        assert torch.equal(eager[i], b[0, 3].permute(1, 2, 0)), (i, idx)
    assert clamped == 4
    cfg2, _ = _cfgs()
    cfg2.use_graph = True
    net2 = _engine(cfg2, sd)
    _, graphed = _sliding_job(net2, clip, passes=3)         # (a configuration is captured the second time it is seen)
    assert any(isinstance(g, torch.cuda.CUDAGraph) for g in net2._graphs.values())
    for i in range(8):
        assert torch.equal(eager[i], graphed[i]), i
    assert net2._att_store.ring.R == 5 and len(net2._att_store.A) == 5


def test_plain_checkpoint_allocates_no_plane(gpu):
    from vfml import build_network, get_cfg
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.decoder_depth, cfg.precision = DEPTH, "f16x3"
    assert cfg.gma is False
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    net.cuda().eval()
    net(_frames(5, 256, 264).cuda(), {})
    assert net.gma is False and net._att_store is None
    assert not [k for k in net._ws if k.startswith("att_")]
    assert net._ws["gru_state"].numel() == 3 * 32 * 33 * 768


# ----------------------------------------------------------------------------- the attention-plane kernel
PLANE_SCALE = 16384.0


def _plane_metrics(plane, P, ref):
    """(row L1 error, row mass error) of an f16 plane [P][ld] holding PLANE_SCALE x probabilities against float64 `ref`."""
    got = plane.hi.view(P, plane.kp)[:, :P].cpu().double() / PLANE_SCALE
    return float((got - ref).abs().sum(1).max()), float((got.sum(1) - 1).abs().max())


@pytest.mark.parametrize("gain", [1.0, 4.0])
@pytest.mark.parametrize("P", [323, 1056, 1100])
def test_attention_plane_against_float64_softmax(gpu, P, gain):
    """hip.attention_plane against softmax in float64, beside the two-call path (split score GEMM to f32, then
    softmax_rows_f16) on the same inputs: at most twice that path's error in either metric - room for another summation
    order and another exp, not for a dropped lo term (about ten times).  gain 4: scores of +-16, the row maximum matters."""
    from vfml import hip
    AD = 128
    ld = (P + 63) // 64 * 64
    g = torch.Generator().manual_seed(P)
    q = (torch.randn(P, AD, generator=g) * gain).contiguous()
    k = (torch.randn(P, AD, generator=g) * gain).contiguous()
    ref = torch.softmax(q.double() @ k.double().T / AD ** 0.5, dim=1)
    dq, dk = q.cuda().view(-1), k.cuda().view(-1)
    # the path that was there before: q as split rows, k as split planes, f32 scores, row softmax to f16
    q16 = torch.empty(P * AD, device="cuda")
    hip.to_s16(dq, P, AD, AD, q16, AD)
    kw = hip.SplitWeight(P, AD, "cuda").fill(dk, scale=16.0)
    scores = torch.empty(P * ld, device="cuda")
    hip.conv2d(q16, AD, AD, 1, 1, P, kw, None, P, 1, 1, scores, ld, out_scale=1.0 / AD ** 0.5, in_fmt=hip.FMT_S16)
    two = hip.PlainWeight(P, ld, "cuda", scale=PLANE_SCALE)
    hip.softmax_rows_f16(scores, P, P, ld, two)
    new = hip.PlainWeight(P, ld, "cuda", scale=PLANE_SCALE)
    new.hi.view(torch.int16).fill_(0x5A5A)
    hip.attention_plane(dq, dk, P, new)
    l1_two, mass_two = _plane_metrics(two, P, ref)
    l1_new, mass_new = _plane_metrics(new, P, ref)
    print(f"[plane] P={P} gain={gain:g}: row L1 {l1_new:.3e} (two-call {l1_two:.3e}), "
          f"row mass {mass_new:.3e} (two-call {mass_two:.3e})")
    assert l1_new <= 2 * l1_two, (l1_new, l1_two)
    assert mass_new <= 2 * mass_two, (mass_new, mass_two)
    assert not new.hi.view(P, ld)[:, P:].any()                      # pad columns
    first = new.hi.clone()
    hip.attention_plane(dq, dk, P, new)
    assert torch.equal(first.view(torch.int16), new.hi.view(torch.int16))


def test_attention_plane_bad_arguments(gpu):
    from ctypes import c_void_p
    from vfml import hip
    P, AD = 70, 128
    q = torch.randn(P * AD, device="cuda")
    ws = torch.empty(2 * P, device="cuda")

    def untouched(plane):
        return bool((plane.hi.view(torch.int16) == 0x5A5A).all())

    good = hip.PlainWeight(P, 128, "cuda", scale=PLANE_SCALE)
    narrow = hip.PlainWeight(P, 96, "cuda", scale=PLANE_SCALE)          # not a multiple of 64
    wide = hip.PlainWeight(2, 32832, "cuda", scale=PLANE_SCALE)         # beyond 32768
    for pl in (good, narrow, wide):
        pl.hi.view(torch.int16).fill_(0x5A5A)
    with pytest.raises(RuntimeError, match="d = 64"):
        hip.attention_plane(q, q, P, good, d=64, workspace=ws)
    with pytest.raises(RuntimeError, match="score_scale nan"):
        hip.attention_plane(q, q, P, good, score_scale=float("nan"), workspace=ws)
    with pytest.raises(RuntimeError, match="ld_plane = 96"):
        hip.attention_plane(q, q, P, narrow, workspace=ws)
    with pytest.raises(RuntimeError, match="ld_plane = 32832"):
        hip.attention_plane(q, q, 2, wide, workspace=ws)
    with pytest.raises(RuntimeError, match="ld_plane = 128"):
        hip.attention_plane(q, q, 129, hip.PlainWeight(129, 128, "cuda"), workspace=torch.empty(258, device="cuda"))
    L = hip.lib()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    for nul in range(4):
        ptrs = [c_void_p(q.data_ptr()), c_void_p(q.data_ptr()), c_void_p(good.hi.data_ptr()), c_void_p(ws.data_ptr())]
        ptrs[nul] = None
        rc = L.vfml_attention_plane_f16(ptrs[0], 128, ptrs[1], 128, P, 128, 0.088, PLANE_SCALE, ptrs[2], 128, ptrs[3], stream)
        assert rc != 0 and b"null pointer" in L.vfml_last_error()
    torch.cuda.synchronize()
    assert untouched(good) and untouched(narrow) and untouched(wide)
    assert hip.attention_plane_workspace_bytes(32400) == 2 * 32400 * 4
