"""forward_interpolate and the warm start off the GPU: the numpy definition of
tests/forward_interpolate_oracle.py - known answers, agreement with scipy's griddata(nearest) on RAFT's recipe, its distance
from the nearest misreadings - the warm oracle stream's cold case, and the host plumbing of the setting."""
import contextlib
import io

import numpy as np
import pytest

import forward_interpolate_oracle as fio


# ----------------------------------------------------------------------------- known answers
def test_zero_and_integer_flows():
    h, w = 5, 7
    out, idx, margin = fio.forward_interpolate(fio.fixture("zero", h, w))
    # row 0 and column 0 land ON the border (x1 = 0 or y1 = 0): strictly invalid, filled from the nearest inner cell
    ys, xs = np.mgrid[0:h, 0:w]
    assert np.array_equal(idx, np.maximum(ys, 1) * w + np.maximum(xs, 1))
    assert not out.any() and out.dtype == np.float32 and idx.dtype == np.int32
    out, idx, _ = fio.forward_interpolate(fio.fixture("uniform:1,-2", h, w))
    # source (xs, ys) lands at (xs + 1, ys - 2): valid for xs <= w - 2 and ys >= 3; target (x, y) takes (x - 1, y + 2) clamped
    want = np.clip(ys + 2, 3, h - 1) * w + np.clip(xs - 1, 0, w - 2)
    assert np.array_equal(idx, want)
    assert np.array_equal(out, np.broadcast_to(np.float32([1, -2]), (h, w, 2)))


def test_ties_go_to_the_lowest_index():
    h, w = 4, 5
    _, idx, margin = fio.forward_interpolate(fio.fixture("uniform:0.5,0", h, w))
    # sources land at (xs + 0.5, ys), row 0 invalid: target x lies midway between the landings of x - 1 and x (d2 = 0.25 both)
    ys, xs = np.mgrid[0:h, 0:w]
    assert np.array_equal(idx, np.maximum(ys, 1) * w + np.maximum(xs - 1, 0))
    assert (margin[:, 1:] == 0).all()                                   # exact ties, in every cell right of column 0
    _, idx, margin = fio.forward_interpolate(fio.fixture("uniform:0.5,0.5", h, w))
    # four sources at equal distance: the lowest is (x - 1, y - 1)
    assert np.array_equal(idx, np.maximum(ys - 1, 0) * w + np.maximum(xs - 1, 0))
    assert (margin[1:, 1:] == 0).all()


def test_duplicates_invalid_and_single_sources():
    h, w = 5, 6
    f = fio.fixture("duplicate", h, w)
    out, idx, margin = fio.forward_interpolate(f)
    lo, hi = (h // 2) * w, (h // 2) * w + 2
    assert (idx == lo).all() and (margin == 0).all()                    # two sources on one point: the lower index everywhere
    assert np.array_equal(out, np.broadcast_to(f.reshape(-1, 2)[lo], (h, w, 2)))
    assert not np.array_equal(f.reshape(-1, 2)[lo], f.reshape(-1, 2)[hi])
    out, idx, margin = fio.forward_interpolate(fio.fixture("all_invalid", h, w))
    assert not out.any() and (idx == -1).all() and np.isinf(margin).all()
    f = fio.fixture("one_valid", h, w)
    out, idx, margin = fio.forward_interpolate(f)
    s = (h // 2) * w + w // 3
    assert (idx == s).all() and np.isinf(margin).all()
    assert np.array_equal(out, np.broadcast_to(np.float32([0.25, 0.375]), (h, w, 2)))
    for hh, ww in ((1, 1), (1, 7), (5, 1)):                            # the degenerate grids of the GPU test: every fixture runs
        for kind in fio.FIXTURES:
            out, idx, _ = fio.forward_interpolate(fio.fixture(kind, hh, ww))
            assert out.shape == (hh, ww, 2) and idx.min() >= -1 and idx.max() < hh * ww


def test_non_finite_entries_are_never_selected():
    for h, w in ((17, 19), (32, 33)):
        f = fio.fixture("nonfinite", h, w)
        bad = ~np.isfinite(f).all(-1).reshape(-1)
        assert bad.sum() > 20 and np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any()
        out, idx, _ = fio.forward_interpolate(f)
        assert idx.min() >= 0 and not bad[idx.reshape(-1)].any() and np.isfinite(out).all()


def test_targets_in_chunks_equal_the_whole_map():
    f = fio.fixture("sigma3", 17, 19)
    out, idx, margin = fio.forward_interpolate(f)
    t = np.array([0, 5, 322, 100, 18, 19])
    o2, i2, m2 = fio.forward_interpolate(f, targets=t, chunk_elems=700)            # two target rows per chunk
    assert np.array_equal(o2, out.reshape(-1, 2)[t]) and np.array_equal(i2, idx.reshape(-1)[t])
    assert np.array_equal(m2, margin.reshape(-1)[t])


def test_float64_flows_are_projected_in_float64():
    f = fio.fixture("sigma3", 17, 19)
    out, idx, _ = fio.forward_interpolate(f.astype(np.float64))
    assert out.dtype == np.float64 and np.array_equal(idx, fio.forward_interpolate(f)[1])


# ----------------------------------------------------------------------------- scipy
def _raft_recipe(flow):
    """RAFT's forward_interpolate on flow [h, w, 2]: scipy.interpolate.griddata(method='nearest') over the landing points
    that stay strictly inside the frame."""
    from scipy import interpolate
    h, w = flow.shape[:2]
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1, y1 = (x0 + flow[..., 0]).reshape(-1), (y0 + flow[..., 1]).reshape(-1)
    ok = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    fx = interpolate.griddata((x1[ok], y1[ok]), flow[..., 0].reshape(-1)[ok], (x0, y0), method="nearest", fill_value=0)
    fy = interpolate.griddata((x1[ok], y1[ok]), flow[..., 1].reshape(-1)[ok], (x0, y0), method="nearest", fill_value=0)
    return np.stack([fx, fy], axis=-1).astype(np.float32)


@pytest.mark.parametrize("kind", ["sigma0.5", "sigma3", "sigma20"])
@pytest.mark.parametrize("h,w", [(17, 19), (32, 33)])
def test_agrees_with_scipy_griddata_nearest(h, w, kind):
    """In every cell whose two nearest sources are more than 1e-6 cells apart (a k-d tree in float64 may break a nearer tie
    another way), the oracle's value is scipy's."""
    pytest.importorskip("scipy")
    f = fio.fixture(kind, h, w)
    out, _, margin = fio.forward_interpolate(f)
    ref = _raft_recipe(f)
    clear = margin > 1e-6
    assert clear.mean() > 0.99
    assert np.array_equal(out[clear], ref[clear])


# ----------------------------------------------------------------------------- the nearest misreadings
def test_the_fixtures_tell_the_definition_from_its_misreadings():
    h, w = 17, 19
    # non-strict validity: with a zero flow row 0 and column 0 would be valid sources, and choose themselves
    f = fio.fixture("zero", h, w)
    assert not np.array_equal(fio.forward_interpolate(f)[1], fio.forward_interpolate(f, strict=False)[1])
    # highest-index tie-break: half-integer flows tie in every cell
    f = fio.fixture("uniform:0.5,0", h, w)
    assert not np.array_equal(fio.forward_interpolate(f)[1], fio.forward_interpolate(f, tie="highest")[1])
    f = fio.fixture("duplicate", h, w)
    assert not np.array_equal(fio.forward_interpolate(f)[0], fio.forward_interpolate(f, tie="highest")[0])
    # a backward (gather) warp and a splat without hole filling: random flows of three cells
    f = fio.fixture("sigma3", h, w)
    out = fio.forward_interpolate(f)[0]
    assert not np.array_equal(out, fio.backward_warp(f))
    assert not np.array_equal(out, fio.no_hole_filling(f))
    assert (fio.no_hole_filling(f) == 0).all(-1).sum() > 20            # the holes are there to be filled


# ----------------------------------------------------------------------------- the warm oracle stream
def test_cold_warm_oracle_is_the_memory_oracle_and_a_warm_field_differs():
    import memflow_memory_oracle as mo
    import memflow_warm_oracle as wo
    import tests_support as ts
    import torch
    from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
    net = ts.memflow_oracle_net(2, seeded_memflow_state_dict(memflow_cfg(), 0))
    clip = mo.fixture_clip(128, 192, frames=3)
    cold = [mo.step(net, clip[:, i:i + 2], [], 0) for i in range(2)]
    st = wo.Stream(net, 0, warm_start=False)
    for i in range(2):
        low, up = st.step(clip[:, i:i + 2])
        assert torch.equal(low, cold[i][0]) and torch.equal(up, cold[i][1]) and st.init is None
    st = wo.Stream(net, 0, warm_start=True)
    low, up = st.step(clip[:, 0:2])
    assert torch.equal(up, cold[0][1]) and st.index is None            # the first field starts cold
    low, up = st.step(clip[:, 1:3], end=True)
    assert st.index is not None and st.index.shape == (16, 24) and wo.epe(up, cold[1][1]) > 0.1
    assert st.low is None                                              # end=True drops the kept flow
    low, up = st.step(clip[:, 1:3])
    assert torch.equal(up, cold[1][1]) and st.index is None


# ----------------------------------------------------------------------------- the entry point's refusals (no launch: no GPU)
def test_argument_validation_needs_no_gpu():
    from vfml import hip
    L = hip.lib()
    assert "vfml_flow_forward_interpolate" in hip.EXPORTS and "warm_start.hip" in hip.SOURCES
    P = 17 * 19
    assert L.vfml_flow_forward_interpolate_workspace_bytes(1, 17, 19) == 8 * P             # one chunk of 2048 sources
    assert L.vfml_flow_forward_interpolate_workspace_bytes(3, 45, 47) == 3 * 2 * 2115 * 8   # two chunks
    assert L.vfml_flow_forward_interpolate_workspace_bytes(1, 0, 19) == 0
    F, O, W = 0x10000, 0x20000, 0x40000                                # never dereferenced: every call below is refused

    def call(fl=F, ld_in=4, n=1, h=17, w=19, o=O, ld_out=4, idx=None, wsp=W, wsb=8 * P):
        return L.vfml_flow_forward_interpolate(fl, ld_in, n, h, w, o, ld_out, idx, wsp, wsb, None)

    for kw, text in ((dict(fl=None), b"null pointer"), (dict(o=None), b"null pointer"), (dict(wsp=None), b"null pointer"),
                     (dict(n=0), b"n = 0"), (dict(h=0), b"h = 0"), (dict(w=-1), b"w = -1"), (dict(h=4097, w=4097), b"2^24"),
                     (dict(ld_in=1), b"ld_in = 1"), (dict(ld_out=1), b"ld_out = 1"), (dict(wsb=8 * P - 8), b"workspace"),
                     (dict(wsp=W + 4), b"workspace"), (dict(n=2), b"workspace"), (dict(fl=F + 2), b"alignment"),
                     (dict(o=F), b"overlaps"), (dict(o=F + 16), b"overlaps")):
        assert call(**kw) != 0, kw
        assert text in L.vfml_last_error(), (kw, L.vfml_last_error())


# ----------------------------------------------------------------------------- host plumbing
def test_setting_and_its_refusals(monkeypatch):
    import flow_processor as fp
    monkeypatch.delenv("VFML_MEMFLOW_WARM_START", raising=False)
    assert fp.MEMFLOW_WARM_START is False and fp.memflow_warm_start() is False
    monkeypatch.setattr(fp, "MEMFLOW_WARM_START", True)
    assert fp.memflow_warm_start() is True
    monkeypatch.setenv("VFML_MEMFLOW_WARM_START", "0")                 # the environment overrides the module setting
    assert fp.memflow_warm_start() is False
    monkeypatch.setattr(fp, "MEMFLOW_WARM_START", False)
    monkeypatch.setenv("VFML_MEMFLOW_WARM_START", "1")
    assert fp.memflow_warm_start() is True
    for bad in ("2", "-1", "yes", "true", "1.0"):
        monkeypatch.setenv("VFML_MEMFLOW_WARM_START", bad)
        with pytest.raises(ValueError, match="VFML_MEMFLOW_WARM_START.*0 or 1"):
            fp.memflow_warm_start()
    monkeypatch.delenv("VFML_MEMFLOW_WARM_START")
    monkeypatch.setattr(fp, "MEMFLOW_WARM_START", 2)
    with pytest.raises(ValueError, match="flow_processor.MEMFLOW_WARM_START"):
        fp.memflow_warm_start()


def test_main_refuses_before_anything_is_computed(tmp_path, monkeypatch):
    import flow_processor as fp
    out = tmp_path / "out"
    out.mkdir()
    argv = ["--input", "synthetic:64x48x4", "--output", str(out), "--device", "cpu", "--model", "memflow"]
    monkeypatch.delenv("VFML_MEMFLOW_MEMORY", raising=False)
    monkeypatch.setenv("VFML_MEMFLOW_WARM_START", "on")
    with pytest.raises(ValueError, match="VFML_MEMFLOW_WARM_START"):
        fp.main(argv)
    monkeypatch.setenv("VFML_MEMFLOW_WARM_START", "1")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = fp.main(argv + ["--tile"])
    assert rc == 1 and "--tile" in buf.getvalue() and "warm start" in buf.getvalue()
    assert not list(out.iterdir())


def test_job_refusals_and_routing():
    from vfml import runner
    runner.check_memory_job(0, True, 8)                                 # neither: nothing to refuse, as before
    runner.check_memory_job(0, True, 8, False)
    runner.check_memory_job(0, False, 1, True)
    with pytest.raises(ValueError, match="warm start.*--tile"):
        runner.check_memory_job(0, True, 1, True)
    with pytest.raises(ValueError, match="warm start.*4 ranks.*cold"):
        runner.check_memory_job(0, False, 4, True)
    with pytest.raises(ValueError, match="memory bank.*--tile"):        # with both the bank's message comes first
        runner.check_memory_job(2, True, 1, True)

    class Proc:
        PAIR_BATCH = 3

        def __init__(self, memory, warm):
            self.memory_frames, self.warm_start, self.calls = memory, warm, []

        def compute_optical_flow_stream(self, clip, idxs):
            self.calls.append(("stream", list(idxs)))
            return [None] * len(idxs)

        def compute_optical_flow_resident_batch(self, clip, idxs):
            self.calls.append(("batch", list(idxs)))
            return [None] * len(idxs)

    assert not runner.warm_start(object()) and not runner.streams(object())
    for memory, warm, route in ((0, False, "batch"), (0, True, "stream"), (2, False, "stream"), (2, True, "stream")):
        p = Proc(memory, warm)
        assert runner.warm_start(p) is warm and runner.streams(p) is (route == "stream")
        list(runner._fields_in_order(p, None, [0, 1, 2, 3]))
        if route == "stream":
            assert p.calls == [("stream", [i]) for i in range(4)]       # a field per pass, in frame order
        else:
            assert p.calls == [("batch", [0, 1, 2]), ("batch", [3])]


def test_cache_directory_names():
    from storage import FlowCacheManager
    from storage.filename_generator import generate_cache_directory
    kw = dict(start_frame=3, max_frames=40, sequence_length=3, model="memflow", dataset="sintel")
    plain = generate_cache_directory("/data/some clip.v2.mp4", **kw)
    assert plain == "/data/some clip.v2_flow_cache_memflow_sintel_seq3_start3_frames40"
    assert generate_cache_directory("/data/some clip.v2.mp4", warm_start=False, **kw) == plain
    assert generate_cache_directory("/data/some clip.v2.mp4", warm_start=True, **kw) == plain + "_warm"
    assert generate_cache_directory("/data/some clip.v2.mp4", memory_frames=2, warm_start=True, **kw) == plain + "_mem2_warm"
    assert generate_cache_directory("/data/some clip.v2.mp4", memory_frames=2, **kw) == plain + "_mem2"
    assert generate_cache_directory("/data/some clip.v2.mp4", fast_mode=True, warm_start=True, **kw).endswith("_fast_warm")
    mgr = FlowCacheManager()
    args = ("/data/c.mp4", 0, 5, 3, False, False, "memflow", "sintel")
    assert mgr.generate_cache_path(*args, warm_start=True) == mgr.generate_cache_path(*args) + "_warm"
    assert mgr.generate_cache_path(*args, memory_frames=2, warm_start=True) == mgr.generate_cache_path(*args) + "_mem2_warm"


def test_processor_carries_the_setting():
    from processing.memflow_inference import MemFlowInference
    from processing.memflow_processor import MemFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        assert MemFlowProcessor("cpu").warm_start is False
        eng = MemFlowInference("cpu", warm_start=True)
        assert eng.get_processor().warm_start is True and eng.get_core_engine().warm_start is True
        assert eng.get_processor().memory_frames == 0
        both = MemFlowProcessor("cpu", memory_frames=2, warm_start=1)
        assert both.memory_frames == 2 and both.warm_start is True
        with pytest.raises(ValueError, match="0 or 1"):
            MemFlowProcessor("cpu", warm_start="yes")
    assert "cold start" in MemFlowProcessor.compute_optical_flow.__doc__         # random access says what it does


def test_stream_and_forward_refuse_bad_arguments_without_a_gpu():
    import torch
    from vfml.memflow_net import MemFlowNetHIP, MemFlowStream, build_memflow_network, memflow_cfg
    net = build_memflow_network(memflow_cfg())
    st = MemFlowStream(net, 0, warm_start=True)
    assert st.warm_start is True and st.flow_size is None and net.stream(1).warm_start is False
    with pytest.raises(ValueError, match="0 or 1"):
        net.stream(0, warm_start="x")
    chk = MemFlowNetHIP._check_flow_init
    dev = torch.device("cpu")
    chk(torch.zeros(1, 2, 16, 24), 1, 16, 24, dev)
    chk(torch.zeros(16, 24, 2), 1, 16, 24, dev)
    with pytest.raises(ValueError, match=r"\[1,2,16,24\] or \[16,24,2\]"):
        chk(torch.zeros(1, 2, 24, 16), 1, 16, 24, dev)
    with pytest.raises(ValueError, match="float32"):
        chk(torch.zeros(16, 24, 2, dtype=torch.float64), 1, 16, 24, dev)
    with pytest.raises(ValueError, match="3 pairs"):
        chk(torch.zeros(16, 24, 2), 3, 16, 24, dev)
    with pytest.raises(ValueError, match="is on"):
        chk(torch.zeros(16, 24, 2), 1, 16, 24, torch.device("cuda:0"))
