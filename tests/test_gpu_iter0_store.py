"""The per-frame store of first-iteration motion features (MOFNetHIP._iter0_store; its bookkeeping, vfml/frame_store.py
Iter0Ring, is tested without a GPU in tests/test_frame_store_cpu.py) and the window set-up pass that feeds it
(vfml_window_seed): a window that takes its older centres' rows from the store gives the bits of the same window computed
from scratch, whatever happened to the store before."""
import contextlib
import io

import pytest
import torch


def _net(seed=0, **over):
    from vfml import build_network, get_cfg
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    for k, v in over.items():
        setattr(cfg, k, v)
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, seed))
    net.cuda().eval()
    return net


def _proc(net, T=5):
    from processing.videoflow_processor import VideoFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=T)
    proc.core.model = net
    return proc


def _clip(nfr, H=128, W=160):
    import numpy as np
    from vfml.synth import synthetic_clip
    return torch.from_numpy(np.stack(synthetic_clip(nfr, H, W))).cuda()


def _scratch(net, proc, clip, i):
    """Field i with no keys: nothing cached, nothing stored."""
    b, _ = net.forward_u8(clip[proc.window_indices(clip.shape[0], i)])
    return b[0, b.shape[1] // 2].permute(1, 2, 0).clone()


def test_window_seed_validates_its_arguments_without_a_gpu():
    from vfml import hip
    L = hip.lib()
    assert L.vfml_window_seed(None, 3, 10, 128, None, 768, 256, 512, 256, None) != 0
    assert b"vfml_window_seed" in L.vfml_last_error()
    assert L.vfml_window_seed(8, 3, 10, 128, 16, 768, 256, 300, 256, None) != 0        # overlapping column blocks
    assert L.vfml_window_seed(8, 17, 10, 128, 16, 768, 256, 512, 256, None) != 0       # more centres than cells
    assert L.vfml_window_seed(8, 3, 10, 126, 16, 768, 256, 512, 256, None) != 0        # cols not whole quads


# ---------------------------------------------------------------------------------------------- the native pass
@pytest.mark.gpu
def test_window_seed_equals_the_torch_copies_on_a_ragged_size(gpu):
    from vfml import hip
    g = torch.Generator(device="cuda").manual_seed(3)
    M, rows, ld, HH, MF = 4, 13 * 7, 768, 256, 512
    state = torch.randn(M * rows * ld, device="cuda", generator=g)
    ctx = [torch.randn(rows * 256, device="cuda", generator=g) for _ in range(M)]
    store = torch.randn(5 * rows * 128, device="cuda", generator=g)
    slots = [store[s * rows * 128:(s + 1) * rows * 128] for s in (3, 0, 4, 1)]
    modes = [hip.SEED_LOAD, hip.SEED_STORE, hip.SEED_NONE, hip.SEED_LOAD]
    want_state, want_store = state.clone().view(M * rows, ld), store.clone()
    want_slots = [want_store[s * rows * 128:(s + 1) * rows * 128] for s in (3, 0, 4, 1)]
    for c in range(M):
        blk = want_state[c * rows:(c + 1) * rows]
        if c != 2:                                    # (centre 2 gets no context map below)
            blk[:, HH:HH + 128].copy_(ctx[c].view(rows, 256)[:, :128])
        if modes[c] == hip.SEED_LOAD:
            blk[:, MF:MF + 128].copy_(want_slots[c].view(rows, 128))
        elif modes[c] == hip.SEED_STORE:
            want_slots[c].view(rows, 128).copy_(blk[:, MF:MF + 128])
    cells = torch.zeros(64, dtype=torch.int64, device="cuda")
    hip.ptr_table_set(cells, [v for c in range(M) for v in (ctx[c] if c != 2 else 0, slots[c], modes[c])])
    hip.window_seed(cells, M, rows, 128, state, ld, HH, MF, 256)
    torch.cuda.synchronize()
    assert torch.equal(state.view(M * rows, ld), want_state)
    assert torch.equal(store, want_store)
    # no slot: the mode is ignored
    before = state.clone()
    hip.ptr_table_set(cells, [v for c in range(M) for v in (0, 0, hip.SEED_LOAD)])
    hip.window_seed(cells, M, rows, 128, state, ld, HH, MF, 256)
    assert torch.equal(state, before)


# ---------------------------------------------------------------------------------------------- the engine
def _straddles(net):
    warm, slots = net.iter0_last
    return bool(warm and slots != sorted(slots))


@pytest.mark.gpu
def test_sliding_job_through_the_store_is_exact(gpu):
    """A sliding job longer than twice the ring (clamped windows at both ends of the clip, windows whose slots straddle the
    ring's end), the same frames in random order, with the store off, after a cleared cache, after a plan change and after
    new weights: every field is the window computed from scratch, bit for bit."""
    import numpy as np
    net = _net()
    nfr = 2 * net.ITER0_RING + 3
    clip = _clip(nfr)
    proc = _proc(net)
    ref = [_scratch(net, proc, clip, i) for i in range(nfr)]
    assert net.iter0_stats == {"warm": 0, "cold": 0}              # (no keys: the store is not involved)
    net.clear_feature_cache()
    straddle = 0
    for i in range(nfr):
        assert torch.equal(proc.compute_optical_flow_resident(clip, i), ref[i]), i
        straddle += _straddles(net)
    assert net.iter0_stats == {"warm": nfr - 1, "cold": 1}        # every window but the first took its older centres' rows
    assert straddle >= 2
    order = np.random.default_rng(0).permutation(nfr)
    for i in order[:12]:
        assert torch.equal(proc.compute_optical_flow_resident(clip, int(i)), ref[int(i)]), int(i)
    assert net.iter0_stats["cold"] > 1                            # (random access misses; correctness does not need a hit)
    net.iter0_store = False
    stats = dict(net.iter0_stats)
    net.clear_feature_cache()
    for i in range(6):
        assert torch.equal(proc.compute_optical_flow_resident(clip, i), ref[i]), i
    assert net.iter0_stats == stats
    net.iter0_store = True
    for i in range(2, 6):                                         # (turned back on: one cold window, then warm ones)
        assert torch.equal(proc.compute_optical_flow_resident(clip, i), ref[i]), i
    net.clear_feature_cache()
    cold = net.iter0_stats["cold"]
    for i in range(4, 8):
        assert torch.equal(proc.compute_optical_flow_resident(clip, i), ref[i]), i
    assert net.iter0_stats["cold"] == cold + 1
    # another arithmetic plan, then other weights: entries of the old ones must not be taken
    net.cfg.precision = "mixed"
    for i in (5, 6, 7, 8):
        a = proc.compute_optical_flow_resident(clip, i).clone()
        assert torch.equal(a, _scratch(net, proc, clip, i)), i
        assert not torch.equal(a, ref[i])
    from vfml.weights import seeded_state_dict
    net.load_state_dict(seeded_state_dict(net.cfg, 1))
    warm = net.iter0_stats["warm"]
    for i in (6, 7, 8, 9):
        a = proc.compute_optical_flow_resident(clip, i).clone()
        assert torch.equal(a, _scratch(net, proc, clip, i)), i
    assert net.iter0_stats["warm"] == warm + 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["full_output", "T3", "T9", "tile", "graph_on", "graph_off", "f16x3", "mixed"])
def test_one_warm_window_each(gpu, case):
    """Four consecutive windows (cold, then warm: run eagerly, captured, replayed) against the same windows from scratch."""
    over = {"graph_on": {"use_graph": True}, "graph_off": {"use_graph": False}, "f16x3": {"precision": "f16x3"},
            "mixed": {"precision": "mixed"}}.get(case, {})
    T = {"T3": 3, "T9": 9}.get(case, 5)
    net = _net(**over)
    proc = _proc(net, T)
    nfr = 14
    clip = _clip(nfr)
    rect = (32, 0, 128, 128) if case == "tile" else None
    pick = case != "full_output"
    for i in range(5, 9):
        ids = proc.window_indices(nfr, i)
        win = clip[ids]
        if rect is not None:
            win = win[:, rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]].contiguous()
        a, _ = net.forward_u8(win, return_lowres=False, frame_keys=[("clip", j, rect) for j in ids], pick_only=pick)
        a = a.clone()
        b, _ = net.forward_u8(win, return_lowres=False, pick_only=pick)
        assert a.shape == b.shape and torch.equal(a, b), (case, i)
    assert net.iter0_stats == ({"warm": 0, "cold": 0} if T == 3 else {"warm": 3, "cold": 1})
