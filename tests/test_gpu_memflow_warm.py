"""The warm start of a MemFlow stream on the GPU: `forward(pair, flow_init=X)`, `stream(M,
warm_start=True)` and the job loop, against the warm oracle stream of tests/memflow_warm_oracle.py.

Depth 4, seed 0, memflow_memory_oracle.fixture_clip, and the bounds of tests/test_gpu_elementwise_memflow.py: every statistic of
tests_support.error_stats (px) and low_stats (cells) of every field stays within K = K_OF['f16x3'] = 8 times N, the float32
oracle's distance from the float64 oracle FOR THE SAME WARM STREAM.  Nothing in a bound comes from the engine.

The projection is a discontinuous selection: a cell whose two nearest landing points are nearly equidistant may choose another
source in float32 than in float64, and the fields after it then differ by a flow value, not by rounding noise.  So every stream
case first asserts, on the oracles alone, the condition under which an elementwise comparison means anything: the float32 and
the float64 oracle stream choose the same source in every cell of every field, and the smallest margin between a cell's best
and second-best source is at least 1e-4 cells (measured on the CPU for these cases: 1.6e-3 and more undrifted, 1.6e-3 at drift 1
with M = 0 and 2.7e-4 with M = 2; the projected flow of the two oracles differs by 5.7e-6 at most; drift 2 falls to 6e-5 and
is left out).  The engine's index map must then EQUAL the oracle's, asserted
before the statistics: a flipped selection is reported as what it is.  Every case prints its PARITY lines before it asserts."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import tests_support as ts

pytestmark = pytest.mark.gpu

DEPTH = 4
PRECISION = "f16x3"
K = ts.K_OF[PRECISION]
MARGIN = 1e-4
_SD, _NETS = {}, {}


def _state(drift=None):
    from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
    if "sd" not in _SD:
        _SD["sd"] = seeded_memflow_state_dict(memflow_cfg(), 0)
    if drift is not None and drift not in _SD:
        _SD[drift] = ts.drift_state_dict(_SD["sd"], drift)
    return _SD["sd" if drift is None else drift]


def _clip(H, W, frames=4):
    import memflow_memory_oracle as mo
    return mo.fixture_clip(H, W, frames=5)[:, :frames].contiguous()


def _engine(drift=None):
    """One engine per set of weights for the module (its workspace follows the frame size)."""
    from vfml.memflow_net import build_memflow_network, memflow_cfg
    if drift not in _NETS:
        cfg = memflow_cfg()
        cfg.decoder_depth = DEPTH
        net = build_memflow_network(cfg)
        net.load_state_dict(_state(drift))
        _NETS[drift] = net.cuda().eval()
    return _NETS[drift]


def _hold(tag, H, W, up, low, r32, l32, r64, l64):
    """One field of the engine (up [1, 2, H, W], low [1, 2, h, w], on the host) against a float64 field, bounded by K times the
    float32 field's distance from it; prints, then asserts."""
    assert up.shape == (1, 2, H, W) and low.shape == (1, 2, H // 8, W // 8)
    assert torch.isfinite(up).all() and torch.isfinite(low).all()
    N, Nl = ts.error_stats(r32, r64), ts.low_stats(l32, l64)
    E, El = ts.error_stats(up[None], r64), ts.low_stats(low[None], l64)
    for what, e, n in (("full", E, N), ("low", El, Nl)):
        print(f"PARITY|memflow-warm-{tag}-{H}x{W}|seed0|{PRECISION}|{what}|N " + " ".join(f"{n[k]:.2e}" for k in ts.STAT_KEYS) +
              "|engine " + " ".join(f"{e[k]:.2e}" for k in ts.STAT_KEYS) + "|ratio " +
              " ".join(f"{e[k] / n[k] if n[k] else float('inf'):.2f}" for k in ts.STAT_KEYS) +
              f"|max |low| {float(l64.abs().max()):.2f} cells")
    return (tag, E, N, El, Nl)


def _assert_held(todo):
    for tag, E, N, El, Nl in todo:
        ts.assert_within(E, N, K, f"[{tag}] field (px)")
        ts.assert_within(El, Nl, K, f"[{tag}] 1/8-resolution flow (cells)")


# ----------------------------------------------------------------------------- forward(pair, flow_init=X)
@pytest.mark.parametrize("H,W", [(136, 152), (256, 264)], ids=["136x152", "256x264"])
def test_forward_with_a_starting_flow(gpu, H, W):
    """X: the float32 warm oracle's projection of field 0's flow - the SAME tensor for the engine and for both oracles (the
    float64 oracle takes X.double()) - starts field 1.  Both accepted layouts give the same bits; a zero X gives the bits of
    flow_init=None."""
    import memflow_warm_oracle as wo
    sd, clip = _state(), _clip(H, W, 3)
    X = wo.oracle_fields(clip, DEPTH, sd, 0, fields=2)["init"]["f32"][1]
    assert X.shape == (1, 2, H // 8, W // 8) and float(X.abs().max()) > 0.2
    pair = clip[:, 1:3]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    l32, r32 = wo.step(ts.memflow_oracle_net(DEPTH, sd), pair, [], 0, X)
    l64, r64 = wo.step(ts.memflow_oracle_net(DEPTH, sd, True), pair.double(), [], 0, X.double())
    net, dpair = _engine(), pair.cuda()
    low, up = (t.clone() for t in net.forward(dpair, flow_init=X.cuda()))
    low2, up2 = net.forward(dpair, flow_init=X[0].permute(1, 2, 0).contiguous().cuda())
    assert torch.equal(low, low2) and torch.equal(up, up2)
    cold = [t.clone() for t in net.forward(dpair)]
    zero = net.forward(dpair, flow_init=torch.zeros_like(X).cuda())
    assert torch.equal(zero[0], cold[0]) and torch.equal(zero[1], cold[1])
    assert not torch.equal(up, cold[1])
    _assert_held([_hold("forward", H, W, up.cpu(), low.cpu(), r32[None], l32[None], r64[None], l64[None])])


def test_forward_refuses_a_bad_starting_flow(gpu):
    net = _engine()
    pair = _clip(128, 192, 2).cuda()
    good = torch.zeros(1, 2, 16, 24, device="cuda")
    before = {k: v.data_ptr() for k, v in net._ws.items()}
    with pytest.raises(ValueError, match=r"\[1,2,16,24\] or \[16,24,2\]"):
        net.forward(pair, flow_init=torch.zeros(1, 2, 24, 16, device="cuda"))
    with pytest.raises(ValueError, match="is on cpu"):
        net.forward(pair, flow_init=good.cpu())
    with pytest.raises(ValueError, match="float32"):
        net.forward(pair, flow_init=good.half())
    with pytest.raises(ValueError, match="2 pairs"):
        net.forward_pairs(_clip(128, 192, 3).cuda(), flow_init=good)
    with pytest.raises(ValueError, match="flow_init is for warm_start=False"):
        net.stream(0, warm_start=True).step(pair, flow_init=good)
    assert {k: v.data_ptr() for k, v in net._ws.items()} == before      # nothing was allocated, let alone launched


# ----------------------------------------------------------------------------- composition
@pytest.mark.parametrize("H,W,M", [(136, 152, 0), (256, 264, 1)], ids=["136x152-M0", "256x264-M1"])
def test_warm_stream_is_its_parts(gpu, H, W, M):
    """stream(M, warm_start=True) over three fields equals, bit for bit, stepping by hand: forward (M = 0) or stream(M) steps
    fed hip.flow_forward_interpolate of the previous field's low-resolution flow."""
    from vfml import hip
    net, clip = _engine(), _clip(H, W).cuda()
    st = net.stream(M, warm_start=True)
    got = [[t.clone() for t in st.step(clip[:, f:f + 2])] for f in range(3)]
    hand = net.stream(M) if M else None
    prev = None
    for f in range(3):
        X = None if prev is None else hip.flow_forward_interpolate(prev[0].permute(1, 2, 0).contiguous())
        pair = clip[:, f:f + 2]
        low, up = hand.step(pair, flow_init=X) if M else net.forward(pair, flow_init=X)
        assert torch.equal(low, got[f][0]) and torch.equal(up, got[f][1]), f
        prev = low.clone()
    if M:
        assert len(st.entries) == len(hand.entries) == M


# ----------------------------------------------------------------------------- the stream against the warm oracle stream
# (H, W, M, drift)
STREAMS = [(128, 192, 0, None), (136, 152, 0, None), (256, 264, 0, None), (256, 264, 1, None), (256, 264, 2, None),
           (256, 264, 0, 1), (256, 264, 2, 1)]


@pytest.mark.parametrize("H,W,M,drift", STREAMS, ids=[f"{c[0]}x{c[1]}-M{c[2]}" + (f"-drift{c[3]}" if c[3] else "") for c in STREAMS])
def test_warm_stream_within_k_times_the_warm_oracles_own_noise(gpu, H, W, M, drift):
    """Three fields through net.stream(M, warm_start=True) against the warm oracle stream of the same capacity.  At drift 1 the
    flow grows to 4, 8.5 and 12.8 cells and half the sources leave the frame."""
    import memflow_warm_oracle as wo
    sd, clip = _state(drift), _clip(H, W)
    ent = wo.oracle_fields(clip, DEPTH, sd, M, fields=3)
    least = wo.stability(ent)                                # the oracles alone: the same source in every cell ...
    print(f"[warm] {H}x{W} M={M} drift={drift}: smallest margin {least:.2e} cells; oracle s f32 {ent['seconds'][0]:.1f} "
          f"f64 {ent['seconds'][1]:.1f}")
    assert least >= MARGIN, least                            # ... and no cell nearer to a flip than this
    net, dclip = _engine(drift), clip.cuda()
    st = net.stream(M, warm_start=True)
    got = []
    for f in range(3):
        low, up = st.step(dclip[:, f:f + 2])
        assert len(st.entries) == min(f + 1, M) and (st.flow_index is None) == (f == 0)
        got.append((low.cpu(), up.cpu(), None if f == 0 else st.flow_index.cpu().numpy().reshape(H // 8, W // 8)))
    net.release_workspace()
    for f in range(1, 3):                                    # a flipped selection is reported as what it is
        flips = int((got[f][2] != ent["index"]["f32"][f]).sum())
        assert flips == 0, f"field {f}: the engine starts {flips} cells from another source than the oracle"
    (r32, l32), (r64, l64) = ent["f32"], ent["f64"]
    tag = f"stream{M}" + (f"-drift{drift}" if drift else "")
    _assert_held([_hold(f"{tag}|field{f}", H, W, got[f][1], got[f][0], ts.field_of(r32, f), ts.field_of(l32, f),
                        ts.field_of(r64, f), ts.field_of(l64, f)) for f in range(3)])


def test_the_warm_start_is_really_on_and_ends_with_the_stream(gpu):
    """256 x 264, M = 0.  Field 1 of a warm stream is more than 0.1 px mean EPE from the COLD oracle's field 1 (the warm and
    cold oracles differ by 0.65 to 0.92 px there).  The field after end=True, and the field after reset(), are held to the cold
    oracle; a pair of another frame size without reset() raises; release_workspace() keeps the flow."""
    import memflow_memory_oracle as mo
    H, W = 256, 264
    sd, clip = _state(), _clip(H, W, 5)
    cold = ts.memflow_oracle_fields(clip, DEPTH, sd, 0)
    (r32, l32), (r64, l64) = cold["f32"], cold["f64"]
    net, dclip = _engine(), clip.cuda()
    st = net.stream(0, warm_start=True)
    st.step(dclip[:, 0:2])
    assert st.flow_size == (H, W)
    _, up = st.step(dclip[:, 1:3], end=True)
    far = mo.epe(up.cpu(), ts.field_of(r32, 1)[0])
    print(f"[warm] field 1 of the warm stream against the cold oracle: {far:.3f} px mean EPE")
    assert far > 0.1, far
    assert st.flow_size is None
    todo = []
    low, up = st.step(dclip[:, 2:4])                                    # after end=True: cold
    assert st.flow_index is None
    todo.append(_hold("after-end|field2", H, W, up.cpu(), low.cpu(), *(ts.field_of(t, 2) for t in (r32, l32, r64, l64))))
    with pytest.raises(ValueError, match="256x264.*128x192.*reset"):
        st.step(dclip[:, 0:2, :, :128, :192].contiguous())
    net.release_workspace()
    assert st.flow_size == (H, W) and st._flow is not None and not st._scratch
    low, up = st.step(dclip[:, 3:5])                                    # the kept flow survived: a warm field
    assert st.flow_index is not None
    st.reset()
    low, up = st.step(dclip[:, 3:5])                                    # after reset(): cold
    assert st.flow_index is None
    todo.append(_hold("after-reset|field3", H, W, up.cpu(), low.cpu(), *(ts.field_of(t, 3) for t in (r32, l32, r64, l64))))
    st.reset()
    st.step(dclip[:, 0:2, :, :128, :192].contiguous())                  # ... and any size forward takes
    _assert_held(todo)


def test_cold_streams_are_unchanged(gpu):
    """warm_start=False: the bits of stream(M) as it is called today - at M = 0 those of forward -, and nothing of the warm
    start is allocated."""
    from vfml.memflow_net import MemFlowStream
    net, clip = _engine(), _clip(256, 264).cuda()
    fwd = [[t.clone() for t in net.forward(clip[:, f:f + 2])] for f in range(3)]
    st0 = net.stream(0, warm_start=False)
    for f in range(3):
        low, up = st0.step(clip[:, f:f + 2])
        assert torch.equal(low, fwd[f][0]) and torch.equal(up, fwd[f][1]), f
    today = MemFlowStream(net, 1)
    ref = [[t.clone() for t in today.step(clip[:, f:f + 2])] for f in range(3)]
    st1 = net.stream(1, warm_start=False)
    for f in range(3):
        low, up = st1.step(clip[:, f:f + 2])
        assert torch.equal(low, ref[f][0]) and torch.equal(up, ref[f][1]), f
    assert not torch.equal(ref[1][1], fwd[1][1])
    for st in (st0, st1, today):
        assert st._flow is None and not st._scratch and st.flow_size is None and st.flow_index is None


# ----------------------------------------------------------------------------- the job loop
def _processor(tmp_path, monkeypatch, memory, warm):
    from processing.memflow_inference import MemFlowInference
    from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
    os.makedirs(tmp_path / "MemFlow_ckpt", exist_ok=True)
    torch.save(seeded_memflow_state_dict(memflow_cfg(), 0), tmp_path / "MemFlow_ckpt" / "MemFlowNet_sintel.pth")
    monkeypatch.chdir(tmp_path)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = MemFlowInference("cuda", sequence_length=3, memory_frames=memory, warm_start=warm)
        eng.load_model()
    return eng.get_processor()


def test_job_walks_one_warm_stream(gpu, tmp_path, monkeypatch):
    """A job over a 6-frame clip at 256 x 264 with the warm start on (no bank) equals stepping the stream by hand over the pairs
    (0, 0), (0, 1), ..., bit for bit, through run_sharded and through compute_optical_flow_stream; continue_stream=True keeps the
    flow across two jobs; a fresh job starts cold; random access stays cold."""
    import memflow_memory_oracle as mo
    from vfml.runner import run_sharded
    x = mo.fixture_clip(256, 264, frames=6)[0]
    frames = [f for f in ((x + 1) * 127.5).round().clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()]
    proc = _processor(tmp_path, monkeypatch, 0, True)
    clip = proc.upload_clip(frames)
    job = run_sharded(proc, clip, range(6))
    core = proc.core_engine
    st = core.model.stream(0, warm_start=True)
    xx = core.normalise_as(torch.from_numpy(np.stack(frames)).cuda().permute(0, 3, 1, 2).float()[None], 0)
    for i in range(6):
        _, up = st.step(xx[:, [max(0, i - 1), i]].contiguous())
        assert np.array_equal(job[i], up[0].permute(1, 2, 0).cpu().numpy()), i
    proc.begin_stream_job()
    direct = proc.compute_optical_flow_stream(clip, range(6))
    for i in range(6):
        assert np.array_equal(job[i], direct[i].cpu().numpy()), i
    first = run_sharded(proc, clip, range(0, 3))
    run_sharded(proc, clip, range(3, 6), prepare_only=True)              # preparing buffers leaves the kept flow alone
    second = run_sharded(proc, clip, range(3, 6), continue_stream=True)
    assert np.array_equal(first, job[:3]) and np.array_equal(second, job[3:])
    fresh = run_sharded(proc, clip, range(3, 6))                         # a job starts cold at its first frame
    random_access = proc.compute_optical_flow_resident(clip, 3).cpu().numpy()
    assert np.array_equal(fresh[0], random_access) and not np.array_equal(fresh[0], job[3])
    assert not np.array_equal(fresh[1], job[4])                          # (another start: another stream from there on)
