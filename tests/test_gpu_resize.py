"""vfml_resize_u8 on the MI355X against the numpy restatement (tests/resize_oracle.py), byte for byte; the ClipFeeder
that resizes behind its uploads; and flow_processor --fast end to end at the reduced resolution."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from test_resize_cpu import IDS, SHAPES, expected, pictures

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("src, dst", SHAPES, ids=IDS)
def test_resize_u8_equals_the_oracle(gpu, src, dst):
    from vfml import hip
    for name, img in pictures(src).items():
        got = hip.resize_u8(torch.from_numpy(img).to(gpu), dst)
        assert got.dtype == torch.uint8 and tuple(got.shape) == dst + (3,)
        np.testing.assert_array_equal(got.cpu().numpy(), expected(src, dst, name), err_msg=name)


def test_own_size_is_a_copy(gpu):
    from vfml import hip
    img = torch.from_numpy(pictures((37, 53), seed=3)["random"]).to(gpu)
    got = hip.resize_u8(img, (37, 53))
    assert got.data_ptr() != img.data_ptr() and torch.equal(got, img)


@pytest.mark.parametrize("src, dst", [((66, 130), (33, 65)), ((131, 262), (64, 130)), ((31, 45), (64, 90))],
                         ids=["2x2", "separable", "enlarge"])
def test_batch_row_slice_and_out_in_a_clip(gpu, src, dst):
    from vfml import hip
    imgs = np.stack([pictures(src, seed=s)["random"] for s in (0, 1, 2)])
    want = np.stack([expected(src, dst, "random", seed=s) for s in (0, 1, 2)])
    dev = torch.from_numpy(imgs).to(gpu)
    # a batch [3,H,W,3], and the same through a clip whose frames are further apart than their bytes
    np.testing.assert_array_equal(hip.resize_u8(dev, dst).cpu().numpy(), want)
    wide = torch.zeros((3, src[0] + 5, src[1], 3), dtype=torch.uint8, device=gpu)
    wide[:, 2:2 + src[0]] = dev
    np.testing.assert_array_equal(hip.resize_u8(wide[:, 2:2 + src[0]], dst).cpu().numpy(), want)
    # a row slice of a larger frame: a pointer offset of an odd number of rows into it
    np.testing.assert_array_equal(hip.resize_u8(wide[1, 2:2 + src[0]], dst).cpu().numpy(), want[1])
    # out= a frame inside a clip: that frame alone is written
    clip = torch.full((4,) + dst + (3,), 7, dtype=torch.uint8, device=gpu)
    ret = hip.resize_u8(dev[2], dst, out=clip[1])
    assert ret.data_ptr() == clip[1].data_ptr()
    got = clip.cpu().numpy()
    np.testing.assert_array_equal(got[1], want[2])
    assert np.all(got[[0, 2, 3]] == 7)
    # out= frames of a clip for a batch
    hip.resize_u8(dev, dst, out=clip[1:4])
    got = clip.cpu().numpy()
    np.testing.assert_array_equal(got[1:4], want)
    assert np.all(got[0] == 7)
    with pytest.raises(ValueError):
        hip.resize_u8(dev, dst, out=clip[0])
    with pytest.raises(ValueError):
        hip.resize_u8(dev[:, :, ::2], dst)
    with pytest.raises(ValueError):
        hip.resize_u8(dev.float(), dst)


def test_clip_feeder_resizes_behind_the_upload(gpu):
    """Five frames through a four-slot ring in two steps: a staging slot is reused, and MemFlow's maxima describe the
    resized frames while the clip is still filling."""
    from vfml.runner import ClipFeeder
    from video import resize_frame
    for src, size in (((200, 320), (100, 160)), ((131, 262), (64, 130))):
        frames = [pictures(src, seed=s)["random"] for s in range(5)]
        small = [resize_frame(f, (size[1], size[0])) for f in frames]
        fd = ClipFeeder(frames, gpu, size=size)
        assert tuple(fd.clip.shape) == (5,) + size + (3,) and ClipFeeder.RING == 4
        assert fd.clip._vfml_frame_maxima[4] == float(small[4].max())
        fd.ensure(2)
        assert fd.clip._vfml_frames_ready == 3
        np.testing.assert_array_equal(fd.clip[:3].cpu().numpy(), np.stack(small[:3]))      # (the current stream waits)
        fd.ensure(4, need=4)
        assert fd.clip._vfml_frames_ready == 5
        for f in range(5):
            np.testing.assert_array_equal(fd.clip[f].cpu().numpy(), small[f], err_msg=str(f))
        fd.reset(frames[::-1])
        fd.ensure(4)
        np.testing.assert_array_equal(fd.clip.cpu().numpy(), np.stack(small[::-1]))


def test_frame_extractor_device_path_equals_the_host_path(gpu, tmp_path):
    """device=: batches through vfml_resize_u8 (more frames than one batch), host arrays back."""
    from video import FrameExtractor, frame_extractor, resize_frame
    frames = np.random.default_rng(7).integers(0, 256, (frame_extractor.DEVICE_BATCH + 3, 131, 262, 3), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", frames)
    with contextlib.redirect_stdout(io.StringIO()):
        got, fps, w, h, start = FrameExtractor(str(tmp_path / "clip.npy"), fast_mode=True, device=gpu).extract_frames()
        one = FrameExtractor(str(tmp_path / "clip.npy"), fast_mode=True, device=gpu).get_frame_at_time(0.1)
    assert (fps, w, h, start) == (30.0, 130, 64, 0) and len(got) == len(frames)
    assert all(isinstance(g, np.ndarray) and g.dtype == np.uint8 for g in got)
    np.testing.assert_array_equal(np.stack(got), np.stack([resize_frame(f, (130, 64)) for f in frames]))
    np.testing.assert_array_equal(one, resize_frame(frames[3], (130, 64)))


def test_composer_resizes_a_device_flow_picture(gpu):
    from video import resize_frame
    from visualization.video_composer import create_side_by_side
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    small = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    want = create_side_by_side(frame, resize_frame(small, (64, 48)))
    got = create_side_by_side(torch.from_numpy(frame).to(gpu), torch.from_numpy(small).to(gpu))
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def _run(argv):
    import flow_processor as fp
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = fp.main(argv)
    assert rc == 0, buf.getvalue()
    return buf.getvalue()


@pytest.fixture()
def workdir(tmp_path, monkeypatch):
    from vfml import get_cfg
    from vfml.weights import write_seeded_checkpoint
    write_seeded_checkpoint(str(tmp_path), get_cfg(), seed=0)
    monkeypatch.chdir(tmp_path)
    return tmp_path


def test_cli_fast_runs_the_job_at_the_reduced_size(gpu, workdir):
    from storage import FlowCacheManager
    from test_render_cpu import read_frames
    from vfml.synth import synthetic_clip
    from video import resize_frame
    base = ["--input", "synthetic:320x200x5", "--fast", "--sequence-length", "3", "--uncompressed"]
    out = workdir / "gpu"
    out.mkdir()
    log = _run(base + ["--output", str(out), "--device", "cuda"])
    assert "Fast mode: aggressive resolution reduction from 320x200 to 160x100 (scale: 0.50)" in log
    (cache,) = [p for p in out.iterdir() if p.is_dir()]
    assert "fast" in cache.name
    mgr = FlowCacheManager()
    assert mgr.check_cache_exists(str(cache), 5)[0]
    for i in range(5):
        f = mgr.load_cached_flow(str(cache), i, 'npz')
        assert f.shape == (100, 160, 2) and f.dtype == np.float32 and np.isfinite(f).all()
    (avi,) = [p for p in out.iterdir() if p.suffix == ".avi"]
    got, info = read_frames(str(avi))
    assert (info["width"], info["height"]) == (320, 100) and len(got) == 5
    for g, f in zip(got, synthetic_clip(5, 200, 320)):
        np.testing.assert_array_equal(g[:, :160], resize_frame(f, (160, 100))[:, :, ::-1])
    # the finished cache rendered by the host path: the identical file
    out2 = workdir / "cpu"
    out2.mkdir()
    log = _run(base + ["--output", str(out2), "--device", "cpu", "--use-flow-cache", str(cache)])
    assert "Using optical flow cache from" in log
    assert (out2 / avi.name).read_bytes() == avi.read_bytes()
    # and by the device path from the complete cache: the feeder that render builds resizes too
    out3 = workdir / "gpu2"
    out3.mkdir()
    _run(base + ["--output", str(out3), "--device", "cuda", "--use-flow-cache", str(cache)])
    assert (out3 / avi.name).read_bytes() == avi.read_bytes()


def test_cli_fast_at_the_smallest_size_the_rule_produces(gpu, workdir):
    """A reduced frame is never below 64 x 128 (a source the rule scales has a longer side above 256, halved at most):
    262x131 -> 130x64 is 8 x 17 cells at 1/8 resolution, three pyramid levels, the padder live."""
    from storage import FlowCacheManager
    out = workdir / "small"
    out.mkdir()
    log = _run(["--input", "synthetic:262x131x4", "--fast", "--sequence-length", "3", "--output", str(out), "--device", "cuda",
                "--interactive", "--skip-lods"])
    assert "from 262x131 to 130x64 (scale: 0.50)" in log
    (cache,) = [p for p in out.iterdir() if p.is_dir()]
    for i in range(4):
        f = FlowCacheManager().load_cached_flow(str(cache), i, 'npz')
        assert f.shape == (64, 130, 2) and np.isfinite(f).all()


def test_cli_without_fast_keeps_the_source_size(gpu, workdir):
    from storage import FlowCacheManager
    out = workdir / "full"
    out.mkdir()
    log = _run(["--input", "synthetic:320x200x5", "--sequence-length", "3", "--uncompressed", "--output", str(out),
                "--device", "cuda", "--interactive"])
    assert "resolution reduction" not in log
    (cache,) = [p for p in out.iterdir() if p.is_dir()]
    for i in range(5):
        assert FlowCacheManager().load_cached_flow(str(cache), i, 'npz').shape == (200, 320, 2)
