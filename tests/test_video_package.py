"""The drop-in's `video` package (VideoInfo, FrameExtractor) over a .npy stack, a synthetic clip and an AVI written by the
project's own writer; ClipFeeder with a target size on the CPU device; and flow_processor's refusal of a cache written
at another resolution."""
import contextlib
import io

import numpy as np
import pytest
import torch

W, H, F = 320, 200, 7


def _frames(n=F, h=H, w=W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """kind -> (path, frames): the same frames as a .npy stack and as an uncompressed AVI (25 fps)."""
    from storage.avi_writer import AviWriter
    d = tmp_path_factory.mktemp("clips")
    frames = _frames()
    np.save(d / "clip.npy", frames)
    wr = AviWriter(str(d / "clip.avi"), 0, 25.0, (W, H))
    for f in frames:
        wr.write(f[:, :, ::-1])
    wr.release()
    frames.setflags(write=False)
    return {"npy": (str(d / "clip.npy"), frames, 30.0), "avi": (str(d / "clip.avi"), frames, 25.0)}


def _quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **k)
    return out, buf.getvalue()


@pytest.mark.parametrize("kind", ["npy", "avi"])
def test_video_info(clips, kind):
    from video import VideoInfo
    path, frames, fps = clips[kind]
    vi = VideoInfo(path)
    info = vi.get_info()
    assert info == {'fps': fps, 'width': W, 'height': H, 'total_frames': F, 'duration_seconds': F / fps, 'path': path}
    assert vi.get_info() is info                                      # cached
    vi.reset_cache()
    assert vi.get_info() is not info and vi.get_info() == info
    assert (vi.get_fps(), vi.get_dimensions(), vi.get_frame_count(), vi.get_duration()) == (fps, (W, H), F, F / fps)
    assert vi.time_to_frame(0.1) == int(0.1 * fps) and vi.frame_to_time(5) == 5 / fps
    assert vi.validate_frame_range(-3, 100) == (0, F) and vi.validate_frame_range(2, 3) == (2, 3)
    with pytest.raises(ValueError, match=f"Start frame {F} exceeds total frames {F}"):
        vi.validate_frame_range(F, 1)
    _, text = _quiet(vi.print_info)
    assert text.splitlines() == [f"Video: {path}", f"Dimensions: {W}x{H}", f"FPS: {fps:.2f}", f"Total frames: {F}",
                                 f"Duration: {F / fps:.2f}s"]


def test_video_info_errors(tmp_path):
    from video import VideoInfo
    with pytest.raises(FileNotFoundError, match="Video file not found: nowhere.npy"):
        VideoInfo("nowhere.npy")
    vi = VideoInfo("synthetic:64x48x9")
    assert vi.get_dimensions() == (64, 48) and vi.get_frame_count() == 9 and vi.get_fps() == 30.0
    vi._info_cache = dict(vi.get_info(), fps=0.0, duration_seconds=None)
    with pytest.raises(ValueError, match="Cannot convert time to frame: invalid FPS"):
        vi.time_to_frame(1.0)
    with pytest.raises(ValueError, match="Cannot convert frame to time: invalid FPS"):
        vi.frame_to_time(1)
    with pytest.raises(ValueError, match="Cannot calculate duration: invalid FPS"):
        vi.get_duration()


def test_flow_processor_shares_the_probing_code():
    import flow_processor as fp
    from video import video_info
    assert fp.time_to_frame is video_info.time_to_frame and fp.validate_frame_range is video_info.validate_frame_range
    assert fp.probe_input("synthetic:64x48x9") == (30.0, 9)


@pytest.mark.parametrize("kind", ["npy", "avi"])
def test_frame_extractor(clips, kind):
    from video import FrameExtractor, resize_frame
    path, frames, fps = clips[kind]
    (got, gfps, w, h, start), text = _quiet(FrameExtractor(path).extract_frames, max_frames=4, start_frame=2)
    assert (gfps, w, h, start) == (fps, W, H, 2) and len(got) == 4
    np.testing.assert_array_equal(np.stack(got), frames[2:6])
    assert text.splitlines() == ["Frame range: 2 to 5"]
    # fast mode: 320x200 halves exactly
    ex = FrameExtractor(path, fast_mode=True)
    (got, gfps, w, h, start), text = _quiet(ex.extract_frames, max_frames=100, start_frame=3)
    assert (gfps, w, h, start) == (fps, 160, 100, 3) and len(got) == F - 3
    assert text.splitlines() == ["Fast mode: aggressive resolution reduction from 320x200 to 160x100 (scale: 0.50)",
                                 f"Frame range: 3 to {F - 1}"]
    for g, f in zip(got, frames[3:]):
        assert g.shape == (100, 160, 3) and g.dtype == np.uint8
        np.testing.assert_array_equal(g, resize_frame(f, (160, 100)))
    # times replace the frame arguments, with the reference's lines
    (got, _, _, _, start), text = _quiet(ex.extract_time_range, 2 / fps + 1e-9, 3 / fps + 1e-9)
    assert start == 2 and len(got) == 3 and text.splitlines()[:2] == [
        f"Start time: {2 / fps + 1e-9}s -> frame 2", f"Duration: {3 / fps + 1e-9}s -> 3 frames"]
    np.testing.assert_array_equal(got[0], resize_frame(frames[2], (160, 100)))
    np.testing.assert_array_equal(ex.get_frame_at_time(4 / fps + 1e-9), resize_frame(frames[4], (160, 100)))
    np.testing.assert_array_equal(FrameExtractor(path).get_frame_at_time(0.0), frames[0])
    with pytest.raises(ValueError, match="Cannot read frame at time 100.0s"):
        ex.get_frame_at_time(100.0)
    with pytest.raises(ValueError, match="exceeds total frames"):
        _quiet(ex.extract_frames, start_frame=F)
    _, text = _quiet(ex.print_extraction_info, 4, 2, fps)
    assert text.splitlines() == [f"Video properties: {W}x{H} @ {fps:.2f} FPS", "Extracting 4 frames starting from frame 2",
                                 "Fast mode: 320x200 -> 160x100 (scale: 0.50)"]


def test_frame_extractor_separable_size_and_the_scale_one_quirk(tmp_path):
    from video import FrameExtractor, resize_frame
    frames = _frames(3, 131, 262, seed=1)
    np.save(tmp_path / "a.npy", frames)
    (got, _, w, h, _), text = _quiet(FrameExtractor(str(tmp_path / "a.npy"), fast_mode=True).extract_frames)
    assert (w, h) == (130, 64) and "from 262x131 to 130x64 (scale: 0.50)" in text
    np.testing.assert_array_equal(np.stack(got), np.stack([resize_frame(f, (130, 64)) for f in frames]))
    # a source the rule does not scale is not resized, and the rule's sides are reported even so
    small = _frames(2, 40, 200, seed=2)
    np.save(tmp_path / "b.npy", small)
    (got, _, w, h, _), _ = _quiet(FrameExtractor(str(tmp_path / "b.npy"), fast_mode=True).extract_frames)
    assert (w, h) == (200, 64)
    np.testing.assert_array_equal(np.stack(got), small)


def test_clip_feeder_with_a_target_size_on_the_cpu_device():
    from vfml.runner import ClipFeeder
    from video import resize_frame
    frames = list(_frames(5, 131, 262, seed=3))
    small = [resize_frame(f, (130, 64)) for f in frames]
    fd = ClipFeeder(frames, "cpu", size=(64, 130))
    assert tuple(fd.clip.shape) == (5, 64, 130, 3) and fd.clip.dtype == torch.uint8
    assert fd.clip._vfml_frames_ready == 0
    maxima = fd.clip._vfml_frame_maxima
    assert len(maxima) == 5 and maxima[4] == float(small[4].max())          # asked before the frame is in the clip
    fd.ensure(1)
    assert fd.clip._vfml_frames_ready == 2
    fd.ensure(10)
    assert fd.clip._vfml_frames_ready == 5
    np.testing.assert_array_equal(fd.clip.numpy(), np.stack(small))
    assert [maxima[i] for i in range(5)] == [float(s.max()) for s in small]
    # the guards, unchanged: frames of one shape - the source's - and a held frame where a window reaches
    with pytest.raises(ValueError, match="one shape"):
        fd.reset(small)
    with pytest.raises(ValueError, match="one shape"):
        fd.reset(frames[:4])
    fd.reset([None, None] + frames[2:])
    fd.ensure(4, need=4)
    assert fd.lo == 2 and fd.next == 5
    np.testing.assert_array_equal(fd.clip[2:].numpy(), np.stack(small[2:]))
    with pytest.raises(RuntimeError, match="was skipped"):
        fd.require(1)
    fd.reset(frames[:3] + [None, None])
    with pytest.raises(RuntimeError, match="not held by this process"):
        fd.ensure(4, need=4)
    # the frames' own size is no target at all; without one the feeder is what it was
    for fd in (ClipFeeder(frames, "cpu"), ClipFeeder(frames, "cpu", size=(131, 262))):
        assert fd.size is None and tuple(fd.clip.shape) == (5, 131, 262, 3)
        fd.ensure(4)
        np.testing.assert_array_equal(fd.clip.numpy(), np.stack(frames))
        assert fd.clip._vfml_frame_maxima[0] == float(frames[0].max())
    with pytest.raises(ValueError):
        ClipFeeder(frames, "cpu", size=(0, 4))


def _write_cache(path, n, h, w):
    from storage import FlowCacheManager
    path.mkdir()
    for i in range(n):
        FlowCacheManager().save_flow_to_cache(np.zeros((h, w, 2), np.float32), str(path), i, 'npz')


def test_stale_cache_of_another_resolution_is_refused(tmp_path):
    """A `fast` cache written at the source's size (before --fast reduced the frames), and a foreign --use-flow-cache."""
    import flow_processor as fp
    np.save(tmp_path / "clip.npy", _frames(3))
    _write_cache(tmp_path / "full", 3, H, W)
    _write_cache(tmp_path / "small", 3, 100, 160)
    base = ["--input", str(tmp_path / "clip.npy"), "--output", str(tmp_path), "--device", "cpu", "--uncompressed",
            "--skip-lods"]
    with pytest.raises(ValueError) as e:
        _quiet(fp.main, base + ["--fast", "--use-flow-cache", str(tmp_path / "full")])
    assert "320x200 fields" in str(e.value) and "160x100" in str(e.value) and "--force-recompute" in str(e.value)
    with pytest.raises(ValueError) as e:
        _quiet(fp.main, base + ["--use-flow-cache", str(tmp_path / "small")])
    assert "160x100 fields" in str(e.value) and "320x200" in str(e.value) and "--force-recompute" in str(e.value)
    assert not [p for p in tmp_path.iterdir() if p.suffix == ".avi"]          # refused before a video is begun


def test_fast_cli_renders_a_reduced_cache_on_the_host(tmp_path):
    """--fast --device cpu over a complete cache at the reduced size: the reference's line, frames resized on the host,
    an AVI of the reduced size whose left tile is the resized frame."""
    import flow_processor as fp
    from test_render_cpu import read_frames
    from video import resize_frame
    frames = _frames(3)
    np.save(tmp_path / "clip.npy", frames)
    _write_cache(tmp_path / "small", 3, 100, 160)
    out = tmp_path / "out"
    out.mkdir()
    rc, text = _quiet(fp.main, ["--input", str(tmp_path / "clip.npy"), "--output", str(out), "--device", "cpu",
                                "--uncompressed", "--skip-lods", "--fast", "--use-flow-cache", str(tmp_path / "small")])
    assert rc == 0, text
    assert "Fast mode: aggressive resolution reduction from 320x200 to 160x100 (scale: 0.50)" in text
    (avi,) = [p for p in out.iterdir() if p.suffix == ".avi"]
    got, info = read_frames(str(avi))
    assert (info["width"], info["height"]) == (320, 100) and len(got) == 3
    for g, f in zip(got, frames):
        np.testing.assert_array_equal(g[:, :160], resize_frame(f, (160, 100))[:, :, ::-1])
