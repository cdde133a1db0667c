"""Batch flow-cache correction (correction_worker.worker_process), CPU side: the numpy oracle against vectors cut from
the reference's own worker (tests/golden/make_correction_fixtures.py), argument checks of the C entry points without
a GPU, the refusal of a CPU device, the CLI and the radius check."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import correction_oracle as co  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "correction.npz"))


def test_fixtures_cover_the_cases():
    scenes = dict(co.fixture_scenes(GOLD))
    recs = np.concatenate([s["records"] for s in scenes.values()])
    assert (recs[:, 9] == 1).any() and (recs[:, 9] == 0).any()                 # fine step taken and skipped
    assert ((recs[:, 9] == 1) & (recs[:, 10] == 0)).any()                      # fine step without a result
    assert ((recs[:, 10] == 1) & (recs[:, 13] > recs[:, 8])).any()             # fine result chosen
    assert (recs[:, 8] == 0).any() and (recs[:, 1] == 0).any()                 # targets outside the frame
    a = scenes["a"]
    assert a["written"] == ["flow_frame_000000.npz", "flow_frame_000002.npz"]  # frame 1: no bad pixel, no file
    assert a["skipped"] == [False, False, False, True]
    assert scenes["b"]["written"] == ["flow_frame_000000.flo", "flow_frame_000001.flo"]


def test_oracle_reproduces_the_reference_worker():
    for tag, sc in co.fixture_scenes(GOLD):
        recs, counts = [], []
        for i in sc["indices"]:
            if i not in sc["flows"]:
                continue
            out, initial, final, r = co.correct_frame(sc["frames"][i], sc["frames"][i + 1], sc["flows"][i],
                                                      co.coarsest_lod(sc, i))
            if initial == 0:
                assert i not in sc["corrected"]
                continue
            counts.append([i, initial, final])
            recs.append(r)
            assert out.tobytes() == sc["corrected"][i].tobytes(), (tag, i, int((out != sc["corrected"][i]).sum()))
        assert counts == sc["counts"], tag
        recs = np.concatenate(recs)
        assert recs.shape == sc["records"].shape
        assert recs[:, :14].tobytes() == sc["records"][:, :14].tobytes(), (tag, np.argwhere(recs[:, :14] != sc["records"][:, :14])[:5])


def test_oracle_primitives():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (50, 50)).astype(np.float32)
    dx, dy = co.phase_correlate(a, np.roll(a, (3, -2), axis=(0, 1)))
    assert abs(dx + 2) < 1e-9 and abs(dy - 3) < 1e-9
    s = rng.integers(0, 256, (50, 60, 3), dtype=np.uint8)
    r = co.match_template(s, s[7:18, 30:41].copy())
    assert r.dtype == np.float32 and r.shape == (40, 50) and np.unravel_index(np.argmax(r), r.shape) == (7, 30)
    assert (co.match_template(s, np.full((11, 11, 3), 9, np.uint8)) == 1).all()      # constant template
    assert co.spiral(11, 11)[:5] == [(0, 0), (1, 0), (1, 1), (0, 1), (-1, 1)] and len(co.spiral(11, 11)) == 121


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from vfml import hip
    L = hip.lib()
    assert L.vfml_flow_correct_workspace_bytes(0, 5) == 0
    assert L.vfml_flow_correct_workspace_bytes(1080, 1920) >= 1080 * 1920 * (3 + 4 + 64)
    p = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below is rejected before a launch
    ws = L.vfml_flow_correct_workspace_bytes(8, 8)

    def call(**kw):
        args = dict(f1=p, f2=p, flow=ctypes.c_void_p(2 << 20), lod=ctypes.c_void_p(3 << 20), lh=8, lw=8, h=8, w=8,
                    tw=p, good=0.8, fine=0.9, rr=25.0, tr=5.5, sr=25.0, out=ctypes.c_void_p(4 << 20), counts=p,
                    rec=None, cap=0, ws=p, wsb=ws)
        args.update(kw)
        return L.vfml_flow_correct(*args.values(), None)

    assert call(f1=None) != 0 and b"null" in L.vfml_last_error()
    assert call(h=0) != 0 and b"bad size" in L.vfml_last_error()
    assert call(tr=4.5) != 0 and b"unsupported radii" in L.vfml_last_error()
    assert call(rr=30.0) != 0 and b"unsupported radii" in L.vfml_last_error()
    assert call(flow=ctypes.c_void_p((2 << 20) + 4)) != 0 and b"aligned" in L.vfml_last_error()
    assert call(out=ctypes.c_void_p(2 << 20)) != 0 and b"alias" in L.vfml_last_error()
    assert call(cap=5) != 0 and b"record" in L.vfml_last_error()
    assert call(wsb=ws - 1) != 0 and b"workspace" in L.vfml_last_error()


def test_no_cpu_path():
    import correction_worker as cw
    sc = dict(co.fixture_scenes(GOLD))["a"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        cw.worker_process(0, [0], sc["frames"], {0: sc["flows"][0]}, {}, "cpu", 5, ["x/flow_frame_000000.npz"], None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cw.correct_flow_cache("/nonexistent", sc["frames"], device="cpu")


def test_unsupported_radii_raise():
    import correction_worker as cw
    for key, val in (("TEMPLATE_RADIUS", 3.5), ("SEARCH_RADIUS", 30), ("DETAIL_ANALYSIS_REGION_SIZE", 16)):
        with pytest.raises(ValueError, match=key):
            cw._constants({key: val})
    assert cw._constants(None) == cw.DEFAULT_CONSTANTS
    assert cw.DEFAULT_CONSTANTS == co.DEFAULT_CONSTANTS


def test_twiddles_match_the_oracle():
    import correction_worker as cw
    assert cw.twiddles().tobytes() == co.twiddles(50).tobytes()


def test_cli_parses_its_flags():
    import correction_worker as cw
    a = cw.parse_args(["--input", "synthetic:64x48x4", "--flow-cache", "/tmp/c", "--start-frame", "1", "--frames", "2"])
    assert (a.input, a.flow_cache, a.start_frame, a.frames, a.device) == ("synthetic:64x48x4", "/tmp/c", 1, 2, "cuda")
    frames = cw._load_frames("synthetic:64x48x3")
    assert len(frames) == 3 and frames[0].shape == (48, 64, 3) and frames[0].dtype == np.uint8
    with pytest.raises(SystemExit):
        cw.parse_args(["--input", "x.npy"])
