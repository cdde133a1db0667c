"""MemFlow's memory bank off the GPU: the oracle of tests/memflow_memory_oracle.py (its memory-free case, known answers, the
separations the GPU discriminators rest on, eviction and clearing) and the host plumbing of the setting."""
import contextlib
import io
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE = {}


def _oracle():
    if "ora" not in _CACHE:
        from oracle import memflow_oracle as mm
        from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
        ora = mm.build_network(mm.get_cfg())
        ora.load_state_dict(seeded_memflow_state_dict(memflow_cfg(), 0))
        _CACHE["ora"] = ora.eval()
    return _CACHE["ora"]


def _fields(H, W, M):
    """The oracle's four fields of the fixture clip at a bank capacity, once per session."""
    import memflow_memory_oracle as mo
    key = (H, W, M)
    if key not in _CACHE:
        _CACHE[key] = mo.run_fields(_oracle(), mo.fixture_clip(H, W), M)
    return _CACHE[key]


def test_memory_free_oracle_is_the_pair_oracle():
    import memflow_memory_oracle as mo
    clip = mo.fixture_clip(128, 192)
    for i, (low, up) in enumerate(_fields(128, 192, 0)):
        low_ref, ref = _oracle()(clip[:, i:i + 2])
        assert torch.equal(low, low_ref) and torch.equal(up, ref), i
    # field 0 of any stream has nothing to read
    for M in (1, 2):
        assert torch.equal(_fields(128, 192, M)[0][1], _fields(128, 192, 0)[0][1])
    assert torch.equal(_fields(128, 192, 2)[1][1], _fields(128, 192, 1)[1][1])         # one entry held either way


def test_known_answers():
    """Sampled values of the fields at 128 x 192 (tests/golden/memflow_memory.json).  5e-5 px: ten times the f32 oracle's
    distance from its float64 form (3e-6 to 6e-6 px, another thread count or convolution algorithm moves it by as much),
    thirty times below the smallest difference between two bank sizes (1.6e-3 px)."""
    with open(os.path.join(HERE, "golden", "memflow_memory.json")) as f:
        J = json.load(f)
    assert J["size"] == [128, 192]
    for M in (0, 1, 2):
        for i, ((_, up), want) in enumerate(zip(_fields(128, 192, M), J["fields"][str(M)])):
            got = [[float(up[0, c, y, x]) for c in (0, 1)] for y, x in J["samples"]]
            assert torch.allclose(torch.tensor(got), torch.tensor(want["at"]), rtol=0, atol=5e-5), (M, i, got, want["at"])
            assert abs(float(up.abs().mean()) - want["mean_abs"]) < 5e-5, (M, i)
            for c in (0, 1):
                assert abs(float(up[0, c].mean()) - want["mean"][c]) < 5e-5, (M, i, c)


def test_bank_sizes_are_apart():
    """What the GPU discriminators (tests/test_gpu_memflow_memory.py) rest on, at 256 x 320, each bound half of what was
    measured: one entry against none at least 5e-3 px on fields 1-3 (measured 1.4e-2), two against one at least 2e-3 px on
    fields 2-3 (measured 4.4e-3, 4.8e-3)."""
    import memflow_memory_oracle as mo
    f0, f1, f2 = (_fields(256, 320, M) for M in (0, 1, 2))
    for i in (1, 2, 3):
        d = mo.epe(f1[i][1], f0[i][1])
        print(f"[memory oracle] 256x320 field {i}: M=1 against M=0 {d:.3e} px")
        assert d >= 5e-3, (i, d)
    for i in (2, 3):
        d = mo.epe(f2[i][1], f1[i][1])
        print(f"[memory oracle] 256x320 field {i}: M=2 against M=1 {d:.3e} px")
        assert d >= 2e-3, (i, d)


def test_eviction_end_and_reset():
    import memflow_memory_oracle as mo
    from oracle import memflow_oracle as mm
    cfg = mm.get_cfg()
    cfg.decoder_depth = 2
    ora = mm.build_network(cfg).eval()
    ora.load_state_dict(_oracle().state_dict())
    clip = mo.fixture_clip(128, 192)
    assert torch.isfinite(ora(clip[:, 0:2])[1]).all()
    st = mo.Stream(ora, 1)
    held = []
    for i in range(4):
        st.step(clip[:, i:i + 2])
        assert len(st.bank) == 1                                   # an M = 1 bank never holds two entries
        held.append(st.bank[0][0].clone())
    assert not torch.equal(held[2], held[3])                       # ... and what it holds is the last field's
    two = mo.Stream(ora, 2)
    for i in range(4):
        two.step(clip[:, i:i + 2])
        assert len(two.bank) == min(i + 1, 2)
    assert torch.equal(two.bank[0][0], held[2]) and torch.equal(two.bank[1][0], held[3])      # oldest first
    _, ref = ora(clip[:, 3:5])
    two.step(clip[:, 2:4], end=True)
    assert not two.bank
    assert torch.equal(two.step(clip[:, 3:5])[1], ref)             # the next field starts from nothing
    assert len(two.bank) == 1
    two.reset()
    assert not two.bank
    assert torch.equal(two.step(clip[:, 3:5])[1], ref)
    zero = mo.Stream(ora, 0)
    zero.step(clip[:, 0:2])
    assert not zero.bank


# ----------------------------------------------------------------------------- host plumbing
def test_cache_directory_names():
    from storage import FlowCacheManager
    from storage.filename_generator import generate_cache_directory
    kw = dict(start_frame=3, max_frames=40, sequence_length=3, model="memflow", dataset="sintel")
    plain = generate_cache_directory("/data/some clip.v2.mp4", **kw)
    assert plain == "/data/some clip.v2_flow_cache_memflow_sintel_seq3_start3_frames40"
    assert generate_cache_directory("/data/some clip.v2.mp4", memory_frames=0, **kw) == plain
    assert generate_cache_directory("/data/some clip.v2.mp4", memory_frames=2, **kw) == plain + "_mem2"
    assert generate_cache_directory("/data/some clip.v2.mp4", fast_mode=True, memory_frames=8, **kw).endswith("_fast_mem8")
    mgr = FlowCacheManager()
    args = ("/data/c.mp4", 0, 5, 3, False, False, "memflow", "sintel")
    assert mgr.generate_cache_path(*args, memory_frames=2) == mgr.generate_cache_path(*args) + "_mem2"


def test_setting_and_its_refusals(monkeypatch):
    import flow_processor as fp
    monkeypatch.delenv("VFML_MEMFLOW_MEMORY", raising=False)
    assert fp.MEMFLOW_MEMORY == 0 and fp.memflow_memory() == 0
    monkeypatch.setattr(fp, "MEMFLOW_MEMORY", 3)
    assert fp.memflow_memory() == 3
    monkeypatch.setenv("VFML_MEMFLOW_MEMORY", "8")                  # the environment overrides the module setting
    assert fp.memflow_memory() == 8
    monkeypatch.setenv("VFML_MEMFLOW_MEMORY", "0")
    assert fp.memflow_memory() == 0
    for bad in ("-1", "9", "x", "1.5"):
        monkeypatch.setenv("VFML_MEMFLOW_MEMORY", bad)
        with pytest.raises(ValueError, match="VFML_MEMFLOW_MEMORY.*0..8"):
            fp.memflow_memory()
    monkeypatch.delenv("VFML_MEMFLOW_MEMORY")
    monkeypatch.setattr(fp, "MEMFLOW_MEMORY", 9)
    with pytest.raises(ValueError, match="flow_processor.MEMFLOW_MEMORY"):
        fp.memflow_memory()


def test_main_refuses_before_anything_is_computed(tmp_path, monkeypatch):
    """A bad setting raises in main() as VFML_MJPG_SAMPLING's does; --tile with a bank is refused with a message.  Neither
    leaves anything behind."""
    import flow_processor as fp
    out = tmp_path / "out"
    out.mkdir()
    argv = ["--input", "synthetic:64x48x4", "--output", str(out), "--device", "cpu", "--model", "memflow"]
    monkeypatch.setenv("VFML_MEMFLOW_MEMORY", "9")
    with pytest.raises(ValueError, match="VFML_MEMFLOW_MEMORY"):
        fp.main(argv)
    monkeypatch.setenv("VFML_MEMFLOW_MEMORY", "2")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = fp.main(argv + ["--tile"])
    assert rc == 1 and "--tile" in buf.getvalue() and "memory" in buf.getvalue()
    assert not list(out.iterdir())


def test_job_refusals():
    from vfml.runner import check_memory_job, memory_frames
    check_memory_job(0, True, 8)                                    # no bank: nothing to refuse
    check_memory_job(2, False, 1)
    with pytest.raises(ValueError, match="--tile"):
        check_memory_job(2, True, 1)
    with pytest.raises(ValueError, match="4 ranks.*empty bank"):
        check_memory_job(2, False, 4)

    class Proc:
        memory_frames = 3
    assert memory_frames(Proc()) == 3 and memory_frames(object()) == 0


def test_processor_carries_the_setting():
    from processing.memflow_inference import MemFlowInference
    from processing.memflow_processor import MemFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        assert MemFlowProcessor("cpu").memory_frames == 0
        eng = MemFlowInference("cpu", memory_frames=2)
        assert eng.get_processor().memory_frames == 2 and eng.get_core_engine().memory_frames == 2
        with pytest.raises(ValueError, match="0..8"):
            MemFlowProcessor("cpu", memory_frames=9)
    assert "empty memory bank" in MemFlowProcessor.compute_optical_flow.__doc__       # random access says what it does
