"""Batch flow-cache correction on the MI355X (vfml_flow_correct through correction_worker): the reference worker's
files, counts and per-pixel intermediates on the fixture scenes (tests/golden/correction.npz), bit for bit; the numpy
oracle's detail records on sampled bad pixels of 1080p and 4K-wide frames, bit for bit; the final count against the
quality map of the returned field; run-to-run identity."""
import contextlib
import io
import os
import re
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
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.gpu
def test_worker_reproduces_the_reference_files(tmp_path):
    import correction_worker as cw
    from storage.cache_manager import FlowFileHandler
    for tag, sc in co.fixture_scenes(GOLD):
        cache = tmp_path / f"{tag}_cache"
        cache.mkdir()
        files = [str(cache / f"flow_frame_{i:06d}.{sc['ext']}") for i in range(len(sc["frames"]))]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = cw.worker_process(0, sc["indices"], sc["frames"], dict(sc["flows"]), dict(sc["lods"]), "cuda:0", 5,
                                    files, dict(cw.DEFAULT_CONSTANTS))
        counts = [[int(m.group(1)), int(m.group(2)), int(m.group(3))] for m in
                  re.finditer(r"Frame\s+(\d+) \| Errors:\s+(\d+) ->\s+(\d+)", buf.getvalue())]
        assert counts == sc["counts"], (tag, counts)
        assert [r["skipped"] for r in res] == sc["skipped"]
        out_dir = tmp_path / f"{tag}_cache_corrected"
        assert sorted(os.listdir(out_dir)) == sc["written"], tag
        for i, want in sc["corrected"].items():
            path = out_dir / f"flow_frame_{i:06d}.{sc['ext']}"
            if sc["ext"] == "npz":
                z = np.load(path)
                assert list(z.keys()) == ["flow"]
                got = z["flow"]
            else:
                assert open(path, "rb").read() == sc["corrected_bytes"][i]
                got = FlowFileHandler.load_flow_flo(str(path))
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (tag, i, int((got != want).sum()))


@pytest.mark.gpu
def test_detail_records_match_the_reference_intermediates():
    import correction_worker as cw
    for tag, sc in co.fixture_scenes(GOLD):
        recs = []
        for i, _, _ in sc["counts"]:
            f1, f2 = _dev(sc["frames"][i]), _dev(sc["frames"][i + 1])
            out, initial, final, r = cw.correct_flow_resident(f1, f2, _dev(sc["flows"][i]), _dev(co.coarsest_lod(sc, i)),
                                                              records=True)
            recs.append(r.cpu().numpy())
        recs = np.concatenate(recs)
        want = sc["records"]
        assert recs.shape == want.shape, tag
        diff = np.argwhere(recs[:, :14] != want[:, :14])
        assert diff.size == 0, (tag, diff[:5], recs[diff[0][0]], want[diff[0][0]])
        best = np.where((recs[:, 10] == 1) & (recs[:, 13] > recs[:, 8]), recs[:, 13], recs[:, 8])
        assert (recs[:, 14] == ((best > 0.8) | (best > recs[:, 1]))).all()


def _perturbed(h, w, seed):
    """Synthetic clip frames plus a flow with noise, slightly and grossly wrong blocks and far-outside vectors."""
    from vfml.synth import synthetic_clip
    frames = synthetic_clip(2, h, w)
    rng = np.random.default_rng(seed)
    flow = (rng.standard_normal((h // 8 + 1, w // 8 + 1, 2)) * 1.5).astype(np.float32)
    flow = np.repeat(np.repeat(flow, 8, 0), 8, 1)[:h, :w].copy()
    flow += (rng.standard_normal((h, w, 2)) * 0.3).astype(np.float32)
    for _ in range(40):
        y, x = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
        flow[y:y + 32, x:x + 32] += (rng.standard_normal(2) * 12).astype(np.float32)
    return frames, flow


def _check_against_oracle(frames, flow, lod, n_sample, seed, extra=()):
    import correction_worker as cw
    from vfml import hip
    f1, f2 = _dev(frames[0]), _dev(frames[1])
    fl, ld = _dev(flow), _dev(lod)
    out, initial, final, rec = cw.correct_flow_resident(f1, f2, fl, ld, records=True)
    torch.cuda.synchronize()
    recs = rec.cpu().numpy()
    got = out.cpu().numpy()
    assert initial == recs.shape[0] > 0
    # the final count is the quality map's red count on the returned field
    assert final == int((hip.flow_quality_map(f1, f2, out, 0.8)[..., 0] > 0).sum().item())
    # only bad pixels change; the list is in raster order
    h, w = flow.shape[:2]
    pix = recs[:, 0].astype(np.int64)
    assert (np.diff(pix) > 0).all()
    changed = np.flatnonzero((got != flow).any(-1).ravel())
    assert np.isin(changed, pix).all()
    # detail records of sampled bad pixels, bit for bit against the oracle
    rng = np.random.default_rng(seed)
    pick = np.unique(np.concatenate([rng.choice(initial, size=min(n_sample, initial), replace=False),
                                     np.asarray(extra, np.int64)]))
    c = dict(co.DEFAULT_CONSTANTS)
    for k in pick:
        p = int(pix[k])
        y, x = divmod(p, w)
        want, vec = co.correct_pixel(frames[0], frames[1], flow, lod, x, y, c)
        assert recs[k].tobytes() == want.tobytes(), (p, recs[k], want)
        if vec is not None:
            assert got[y, x].tobytes() == np.array(vec, np.float32).tobytes(), p
        else:
            assert got[y, x].tobytes() == flow[y, x].tobytes(), p
    # run to run
    out2, i2, f2_, rec2 = cw.correct_flow_resident(f1, f2, fl, ld, records=True)
    assert (i2, f2_) == (initial, final)
    assert torch.equal(out2, out) and torch.equal(rec2, rec)
    return recs, pick


@pytest.mark.gpu
def test_1080p_records_match_the_oracle():
    from storage.cache_manager import LODGenerator
    frames, flow = _perturbed(1080, 1920, 5)
    lod = LODGenerator.generate_lods(flow, 5)[4]
    recs, pick = _check_against_oracle(frames, flow, lod, 2000, 11)
    assert len(pick) >= 2000
    assert (recs[:, 9] == 1).any() and (recs[:, 10] == 1).any() and (recs[:, 14] == 1).any()


@pytest.mark.gpu
def test_4k_wide_frame():
    """3840-wide frames, with blocks whose vectors send the coarse target far to the left of the frame: the
    search-area slice gets a negative stop and spans nearly the whole width."""
    frames, flow = _perturbed(2160, 3840, 7)
    flow[1000:1004, 3000:3100] = [3400.0, 0.0]
    recs, pick = _check_against_oracle(frames, flow, flow, 150, 13, extra=())
    # the far-left block: records for some of its pixels, with a fine step over a wide area
    pix = recs[:, 0].astype(np.int64)
    block = np.flatnonzero(np.isin(pix, [1001 * 3840 + x for x in range(3000, 3100, 9)]))
    assert block.size > 0
    _check_against_oracle(frames, flow, flow, 0, 0, extra=block[:6])


@pytest.mark.gpu
def test_correct_flow_cache_1080p_reads_back(tmp_path):
    """A 1080p synthetic .npz cache with engine LODs, corrected through the CLI's function and through the CLI itself:
    the _corrected directory holds one file per frame with bad pixels, FlowCacheManager reads them back, and they are
    the fields correct_flow_resident returns."""
    import subprocess
    import correction_worker as cw
    from storage.cache_manager import FlowCacheManager
    from vfml.synth import synthetic_clip
    h, w = 1080, 1920
    frames = synthetic_clip(3, h, w)
    mgr = FlowCacheManager()
    cache = tmp_path / "cache"
    rng = np.random.default_rng(2)
    flows = []
    for i in range(2):
        fl = np.zeros((h, w, 2), np.float32)
        fl[100 * (i + 1):100 * (i + 1) + 64, 300:500] = [9.0, -4.0]
        fl[700:720, 1800:1900] = [0.5, 30.0]
        fl += (rng.standard_normal((h, w, 2)) * 0.4).astype(np.float32)
        mgr.save_flow_to_cache(fl, str(cache), i, "npz")
        mgr.save_flow_lods(mgr.lod_generator.generate_lods(fl, 5), str(cache), i)
        flows.append(fl)
    with contextlib.redirect_stdout(io.StringIO()):
        res = cw.correct_flow_cache(str(cache), frames)
    assert [r["skipped"] for r in res] == [False, False] and all(r["initial"] > 0 for r in res)
    out_dir = str(cache) + "_corrected"
    assert sorted(os.listdir(out_dir)) == ["flow_frame_000000.npz", "flow_frame_000001.npz"]
    for i in range(2):
        back = mgr.load_cached_flow(out_dir, i)
        lod = mgr.load_flow_lod(str(cache), i, 4)
        want, initial, final = cw.correct_flow_resident(_dev(frames[i]), _dev(frames[i + 1]), _dev(flows[i]), _dev(lod))
        assert back.dtype == np.float32 and back.tobytes() == want.cpu().numpy().tobytes()
        assert (initial, final) == (res[i]["initial"], res[i]["final"]) and final < initial
    # the CLI, on the same cache (frames regenerated from the synthetic: spec)
    for name in os.listdir(out_dir):
        os.remove(os.path.join(out_dir, name))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "video-flow-ml_amd", "correction_worker.py"), "--input",
                        f"synthetic:{w}x{h}x3", "--flow-cache", str(cache), "--start-frame", "1", "--frames", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Frame    1 | Errors:" in r.stdout and "corrected 1 of 1 frames" in r.stdout
    assert os.listdir(out_dir) == ["flow_frame_000001.npz"]
    assert mgr.load_cached_flow(out_dir, 1).tobytes() == np.load(os.path.join(out_dir, "flow_frame_000001.npz"))["flow"].tobytes()
