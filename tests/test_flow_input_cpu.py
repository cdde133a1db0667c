"""--flow-input on the host: the decoders, the difference overlay, the 2x3 grid and flow_processor's comparison mode
against the reference's own process_video (tests/golden/flow_input.npz, make_flow_input_fixtures.py), byte for byte;
the AVI reader; the argument errors; and the drop-in reading back its own --flow-only video."""
import contextlib
import io
import os

import numpy as np
import pytest

from test_render_cpu import GOLD, parse_avi, read_frames

FX = np.load(os.path.join(os.path.dirname(__file__), "golden", "flow_input.npz"))
JOBS = {"rg8_6": "motion-vectors-rg8", "rgb8_6": "motion-vectors-rgb8", "rg8_4": "motion-vectors-rg8",
        "rgb8_8": "motion-vectors-rgb8"}
OVERLAYS = ("40x56", "20x300", "37x53")
CLAMP = 32.0


# ---- 1. the host functions against the reference-cut arrays ------------------------------------------------------------
@pytest.mark.parametrize("variant", ["rg8", "rgb8"])
@pytest.mark.parametrize("clamp", [32.0, 7.3])
def test_host_decoder_matches_reference(variant, clamp):
    from encoding.flow_encoders import decode_motion_vectors
    got = decode_motion_vectors(FX["decode_in"], clamp_range=clamp, format_variant=variant)
    ref = FX[f"decode_{variant}_{clamp}"]
    assert got.dtype == ref.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", OVERLAYS)
def test_host_difference_overlay_matches_reference(name):
    from visualization.video_composer import create_difference_overlay
    a, b, ref = FX[f"overlay_a_{name}"], FX[f"overlay_b_{name}"], FX[f"overlay_{name}"]
    got = create_difference_overlay(a, b)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, ref)
    # the fixture holds what it says: bounds and neighbours, NaN -> black, every class, a legend clipped at the top
    assert got[3, 0].tolist() == [0, 0, 0] and got[3, 1].tolist() == [0, 0, 0] and got[3, 4].tolist() == [0, 0, 0]
    classes = [[0, 255, 0]] * 2 + [[255, 255, 0]] * 3 + [[255, 165, 0]] * 3 + [[255, 0, 0]] * 3 + [[255, 0, 255]]
    assert got[0, :9].tolist() == classes[:9]
    if name == "20x300":            # h - 20 = 0: the squares' top 12 rows are cut off, rows 0 and 1 remain
        assert got[0, 9:24].tolist() == [[255, 255, 255]] + [[0, 255, 0]] * 13 + [[255, 255, 255]]
        assert got[1, 9:24].tolist() == [[255, 255, 255]] * 15 and got[0, 100:113].tolist() == [[255, 165, 0]] * 13
        assert got[0, 190:203].tolist() == [[255, 0, 255]] * 13 and not np.all(got[2, 9:24] == 255)
    else:
        assert got[0, :12].tolist() == classes


def host_loop(job):
    """The reference's --taa --flow-input loop (process_video :958-1130) on the host functions."""
    from effects.taa_processor import TAAProcessor
    from encoding.flow_encoders import decode_motion_vectors
    from visualization.video_composer import create_6_video_grid, create_difference_overlay
    import flow_processor as fp
    frames, fields, video = GOLD["frames"], GOLD["fields"], FX[f"video_{job}"]
    h, w = frames.shape[1:3]
    fmt = JOBS[job]
    enc = fp.render_encoder(fmt, CLAMP)
    t1, t2, t3 = TAAProcessor(alpha=0.1), TAAProcessor(alpha=0.1), TAAProcessor(alpha=0.1)
    prev, out = None, []
    for i in range(len(frames)):
        ext = decode_motion_vectors(video[min(i, len(video) - 1)][h:], clamp_range=CLAMP,
                                    format_variant=fp.FLOW_INPUT_VARIANTS[fmt])
        a = t1.apply_taa(frames[i], flow_pixels=prev, alpha=0.1, use_flow=True, sequence_id='flow_taa')
        b = t2.apply_taa(frames[i], flow_pixels=None, alpha=0.1, use_flow=False, sequence_id='simple_taa')
        c = t3.apply_taa(frames[i], flow_pixels=ext, alpha=0.1, use_flow=True, sequence_id='external_taa')
        prev = fields[i]
        out.append(create_6_video_grid(frames[i], enc.encode(ext, w, h), a, b, c,
                                       create_difference_overlay(fields[i], ext)))
    return np.stack(out)


@pytest.mark.parametrize("job", list(JOBS))
def test_host_grid_matches_reference(job):
    ours, ref = host_loop(job), FX[f"out_{job}"]
    assert ours.shape == ref.shape and ours.dtype == np.uint8
    np.testing.assert_array_equal(ours, ref)


def test_rectangle_definition():
    from visualization.video_composer import fill_rectangle
    img = np.zeros((6, 8), np.uint8)
    fill_rectangle(img, (2, 1), (4, 3), 7)
    assert img.sum() == 7 * 9 and img[1:4, 2:5].all()             # both corners inclusive
    fill_rectangle(img, (6, -3), (11, 0), 9)
    assert (img == 9).sum() == 2 and img[0, 6] == img[0, 7] == 9  # clipped to the picture
    before = img.copy()
    fill_rectangle(img, (9, 9), (12, 12), 5)
    fill_rectangle(img, (0, -5), (3, -1), 5)
    np.testing.assert_array_equal(img, before)                    # wholly outside: nothing


# ---- 2. the command line ----------------------------------------------------------------------------------------------
def write_case(tmp_path):
    from storage import FlowCacheManager
    clip = str(tmp_path / "clip.npy")
    np.save(clip, GOLD["frames"])
    cache = tmp_path / "cache"
    cache.mkdir()
    for i, f in enumerate(GOLD["fields"]):
        FlowCacheManager().save_flow_to_cache(f, str(cache), i, 'npz')
    return clip, str(cache)


def write_flow_video(tmp_path, frames, kind, name="flowvideo"):
    """RGB frames -> a `.npy` stack or an uncompressed `.avi` written by AviWriter."""
    from storage.avi_writer import AviWriter
    if kind == "npy":
        path = str(tmp_path / f"{name}.npy")
        np.save(path, frames)
        return path
    path = str(tmp_path / f"{name}.avi")
    wr = AviWriter(path, 0, 30.0, (frames.shape[2], frames.shape[1]))
    for f in frames:
        wr.write(f[:, :, ::-1])
    wr.release()
    return path


def run_cli(tmp_path, device, clip, cache, extra, out_name="out"):
    """flow_processor.main on a complete cache -> (avi path, stdout)."""
    import flow_processor as fp
    out = tmp_path / out_name
    out.mkdir()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = fp.main(["--input", clip, "--output", str(out), "--device", device, "--skip-lods", "--uncompressed",
                      "--use-flow-cache", cache] + extra)
    assert rc == 0, buf.getvalue()
    avis = sorted(os.listdir(out))
    assert len(avis) == 1 and avis[0].endswith(".avi"), avis
    return str(out / avis[0]), buf.getvalue()


def run_flow_input_job(tmp_path, device, job, kind, out_name="out"):
    clip, cache = write_case(tmp_path) if not (tmp_path / "clip.npy").exists() else \
        (str(tmp_path / "clip.npy"), str(tmp_path / "cache"))
    flow_video = write_flow_video(tmp_path, FX[f"video_{job}"], kind, name=f"flowvideo_{out_name}")
    return run_cli(tmp_path, device, clip, cache, ["--taa", "--flow-input", flow_video, "--flow-format", JOBS[job],
                                                   "--motion-vectors-clamp-range", str(CLAMP)], out_name)


def log_block(log):
    lines = log.splitlines()
    at = lines.index("[Flow Input] Extracting flow from external video...")
    end = lines.index("", at)
    return lines[at:end]


@pytest.mark.parametrize("kind", ["npy", "avi"])
@pytest.mark.parametrize("job", list(JOBS))
def test_cli_flow_input_writes_the_reference_video(tmp_path, job, kind):
    path, log = run_flow_input_job(tmp_path, "cpu", job, kind)
    got, info = read_frames(path)
    ref = FX[f"out_{job}"]
    h, w = GOLD["frames"].shape[1:3]
    assert (info["width"], info["height"]) == (2 * w, 3 * h) and info["dmlh_frames"] == len(ref)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got, ref)
    assert log_block(log) == [str(s) for s in FX[f"log_{job}"]]
    assert "concerns video composition" not in log


# ---- 3. the AVI reader ------------------------------------------------------------------------------------------------
def test_avi_reader_round_trip_over_opendml_segments(tmp_path):
    from storage import avi_reader
    from storage.avi_writer import AviWriter
    rng = np.random.default_rng(3)
    w, h, n = 37, 21, 13                                     # odd width: every DIB row is padded
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    path = str(tmp_path / "raw.avi")
    wr = AviWriter(path, 0, 24.0, (w, h), segment_bytes=12000)
    for f in frames:
        wr.write(f[:, :, ::-1])
    wr.release()
    assert len(parse_avi(path)["riff"]) >= 3                 # several AVIX segments
    assert avi_reader.probe(path) == {"frames": n, "fps": 24.0, "width": w, "height": h, "codec": "BI_RGB"}
    with avi_reader.AviReader(path) as r:
        assert (r.frame_count, r.fps, r.width, r.height) == (n, 24.0, w, h)
        for k in range(n):
            np.testing.assert_array_equal(r.read(), frames[k], err_msg=str(k))
        assert r.read() is None and r.read() is None
    np.testing.assert_array_equal(np.stack(avi_reader.read_frames(path, 9, 100)), frames[9:])
    np.testing.assert_array_equal(np.stack(avi_reader.read_frames(path, 2, 3)), frames[2:5])


def test_avi_reader_probe_does_not_decode(tmp_path):
    """Headers only: the file may end right behind them."""
    from storage import avi_reader
    from storage.avi_writer import AviWriter
    path = str(tmp_path / "raw.avi")
    wr = AviWriter(path, 0, 25.0, (16, 8))
    for k in range(7):
        wr.write(np.full((8, 16, 3), k, np.uint8))
    wr.release()
    buf = open(path, 'rb').read()
    cut = str(tmp_path / "cut.avi")
    open(cut, 'wb').write(buf[:buf.index(b'movi') + 4])
    assert avi_reader.probe(cut) == {"frames": 7, "fps": 25.0, "width": 16, "height": 8, "codec": "BI_RGB"}


def test_avi_reader_mjpg_equals_pillow(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    from storage import avi_reader
    from storage.avi_writer import AviWriter
    yy, xx = np.mgrid[0:48, 0:64]
    frames = [np.stack([xx * 3 + 9 * i, yy * 4, (xx + yy) * 2], 2).astype(np.uint8) for i in range(5)]
    path = str(tmp_path / "mjpg.avi")
    wr = AviWriter(path, 'MJPG', 30.0, (64, 48), workers=3)
    for f in frames:
        wr.write(f[:, :, ::-1])
    wr.release()
    assert avi_reader.probe(path) == {"frames": 5, "fps": 30.0, "width": 64, "height": 48, "codec": "MJPG"}
    got = avi_reader.read_frames(path)
    chunks = parse_avi(path)["frames"]
    assert len(got) == len(chunks) == 5
    for g, data, f in zip(got, chunks, frames):
        np.testing.assert_array_equal(g, np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
        assert np.abs(g.astype(int) - f.astype(int)).mean() < 4      # and it is the picture, RGB


def test_avi_reader_rejects_unknown_codec(tmp_path):
    from storage import avi_reader
    from storage.avi_writer import AviWriter
    path = str(tmp_path / "raw.avi")
    wr = AviWriter(path, 0, 25.0, (16, 8))
    wr.write(np.zeros((8, 16, 3), np.uint8))
    wr.release()
    buf = bytearray(open(path, 'rb').read())
    at = buf.index(b'strf') + 8 + 16
    assert buf[at:at + 4] == b'\0\0\0\0'
    buf[at:at + 4] = b'H264'
    open(path, 'wb').write(bytes(buf))
    assert avi_reader.probe(path)["codec"] == "H264"
    with pytest.raises(ValueError, match="unsupported codec 'H264'"):
        avi_reader.AviReader(path)
    with pytest.raises(ValueError, match="not an AVI"):
        open(path, 'wb').write(b'RIFF\x04\0\0\0WAVE')
        avi_reader.probe(path)


def test_input_clip_may_be_an_avi_of_our_own(tmp_path):
    """probe_input / load_frames read .avi files through the reader when OpenCV is not importable."""
    import flow_processor as fp
    try:
        import cv2  # noqa: F401
        pytest.skip("OpenCV present: it reads the file, as before")
    except ImportError:
        pass
    path = write_flow_video(tmp_path, GOLD["frames"], "avi", name="clip")
    assert fp.probe_input(path) == (30.0, 6)
    frames, fps, w, h, start = fp.load_frames(path, 2, 3)
    assert (fps, w, h, start) == (30.0, 56, 40, 2)
    np.testing.assert_array_equal(np.stack(frames), GOLD["frames"][2:5])


# ---- 4. errors, and the flag without --taa ----------------------------------------------------------------------------
def test_flow_input_errors(tmp_path):
    import flow_processor as fp
    clip, cache = write_case(tmp_path)
    base = ["--input", clip, "--output", str(tmp_path), "--device", "cpu", "--skip-lods", "--uncompressed",
            "--use-flow-cache", cache]
    good = write_flow_video(tmp_path, FX["video_rg8_6"], "npy")
    missing = str(tmp_path / "nothing.avi")
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match=f"Flow input video not found: {missing}"):
            fp.main(base + ["--taa", "--flow-input", missing, "--flow-format", "motion-vectors-rg8"])
        for taa in ([], ["--taa"]):
            with pytest.raises(ValueError, match="Unsupported flow format: hsv"):
                fp.main(base + taa + ["--flow-input", good, "--flow-format", "hsv"])
        other = write_flow_video(tmp_path, np.zeros((6, 64, 48, 3), np.uint8), "avi", name="other")
        with pytest.raises(ValueError) as e:
            fp.main(base + ["--taa", "--flow-input", other, "--flow-format", "motion-vectors-rg8"])
        assert "48x32" in str(e.value) and "56x40" in str(e.value)
    assert not any(n.endswith(".avi") and n not in ("other.avi",) for n in os.listdir(tmp_path))   # nothing rendered


def test_flow_input_without_taa_renders_the_ordinary_video(tmp_path):
    clip, cache = write_case(tmp_path)
    flow_video = write_flow_video(tmp_path, FX["video_rg8_6"], "npy")
    fmt = ["--flow-format", "motion-vectors-rg8"]
    plain, _ = run_cli(tmp_path, "cpu", clip, cache, fmt, "plain")
    with_flag, log = run_cli(tmp_path, "cpu", clip, cache, fmt + ["--flow-input", flow_video], "flag")
    assert open(plain, 'rb').read() == open(with_flag, 'rb').read()
    assert "[Flow Input]" not in log and "without --taa" in log
    stacked, _ = run_cli(tmp_path, "cpu", clip, cache, fmt + ["--flow-only", "--taa"], "stacked")
    stacked_flag, log = run_cli(tmp_path, "cpu", clip, cache, fmt + ["--flow-only", "--taa", "--flow-input", flow_video],
                                "stacked_flag")
    assert open(stacked, 'rb').read() == open(stacked_flag, 'rb').read()
    assert sum("--flow-only" in ln and "--flow-input" in ln for ln in log.splitlines()) == 1


# ---- 5. the drop-in reads its own output --------------------------------------------------------------------------------
def legend_mask(h, w):
    from visualization.video_composer import fill_rectangle
    m = np.zeros((h, w), np.uint8)
    for i in range(5):
        fill_rectangle(m, (10 + 45 * i - 1, h - 33), (10 + 45 * i + 13, h - 19), 1)
    return m.astype(bool)


def own_round_trip(tmp_path, device, fmt):
    clip, cache = write_case(tmp_path)
    first, _ = run_cli(tmp_path, device, clip, cache, ["--flow-only", "--flow-format", fmt], "first")
    second, log = run_cli(tmp_path, device, clip, cache, ["--taa", "--flow-input", first, "--flow-format", fmt], "second")
    got, _ = read_frames(second)
    return got[:, :, :, ::-1], log          # RGB


@pytest.mark.parametrize("fmt", ["motion-vectors-rg8", "motion-vectors-rgb8"])
def test_own_flow_only_video_as_flow_input(tmp_path, fmt):
    """The encoder truncates: each decoded component lies in (v - 64/255, v] for |v| <= 32 (the fixture fields stay
    inside +-26 px), so the difference magnitude stays below 0.251 * sqrt(2) = 0.355 < 0.5: outside the legend every
    pixel of the difference tile is green or yellow."""
    rgb, log = own_round_trip(tmp_path, "cpu", fmt)
    h, w = GOLD["frames"].shape[1:3]
    assert rgb.shape == (6, 3 * h, 2 * w, 3) and "  Flow input has 6 frames" in log
    np.testing.assert_array_equal(rgb[:, :h, :w], GOLD["frames"])
    diff = rgb[:, 2 * h:, w:][:, ~legend_mask(h, w)]
    green = np.all(diff == (0, 255, 0), axis=-1)
    yellow = np.all(diff == (255, 255, 0), axis=-1)
    assert np.all(green | yellow), (~(green | yellow)).sum()
    assert green.any() and yellow.any()
