"""vfml_jpeg_encode_rgb on the MI355X against the numpy restatement (tests/jpeg_oracle.py), byte for byte: the pictures of
test_jpeg_cpu.py, strided input, placement in a larger buffer, a capacity that is too small, and the MJPG files of
flow_processor and flow_maps end to end."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import jpeg_oracle as jo
from test_jpeg_cpu import PICTURES, oracle_file

pytestmark = pytest.mark.gpu


def gpu_file(hip, img, quality=95, **kw):
    scan, length = hip.jpeg_encode(img, quality, **kw)
    h, w = img.shape[:2]
    return hip.jpeg_file(hip.jpeg_header(h, w, quality), hip.jpeg_scan(scan, length))


@pytest.mark.parametrize("name", list(PICTURES))
def test_stream_equals_the_oracle(gpu, name):
    from vfml import hip
    got = gpu_file(hip, torch.from_numpy(PICTURES[name]).to(gpu))
    want = oracle_file(name)
    assert len(got) == len(want), (len(got), len(want))
    assert got == want


@pytest.mark.parametrize("quality", [50, 100])
def test_other_qualities(gpu, quality):
    from vfml import hip
    img = PICTURES["random45x67"]
    assert gpu_file(hip, torch.from_numpy(img).to(gpu), quality) == jo.encode(img, quality)


def test_row_slice_of_a_larger_buffer(gpu):
    from vfml import hip
    img = PICTURES["random45x67"]
    h, w = img.shape[:2]
    big = torch.full((h + 8, w + 13, 3), 201, dtype=torch.uint8, device=gpu)
    big[3:3 + h, :w] = torch.from_numpy(img).to(gpu)
    view = big[3:3 + h, :w]                        # row stride 3 (w + 13) > 3 w, an odd row offset
    assert view.stride(0) == 3 * (w + 13) and not view.is_contiguous()
    assert gpu_file(hip, view) == oracle_file("random45x67")


def test_out_inside_a_larger_buffer(gpu):
    from vfml import hip
    want = oracle_file("noise150x40")
    n = len(want) - len(hip.jpeg_header(150, 40, 95)) - 2
    buf = torch.full((n + 64 + 37,), 0xA5, dtype=torch.uint8, device=gpu)
    scan, length = hip.jpeg_encode(torch.from_numpy(PICTURES["noise150x40"]).to(gpu), out=buf[37:37 + n + 5])
    assert scan.data_ptr() == buf.data_ptr() + 37 and int(length.item()) == n
    host = buf.cpu().numpy()
    assert hip.jpeg_file(hip.jpeg_header(150, 40, 95), host[37:37 + n].tobytes()) == want
    assert np.all(host[:37] == 0xA5) and np.all(host[37 + n:] == 0xA5)


def test_capacity_too_small(gpu):
    from vfml import hip
    want = oracle_file("noise150x40")
    n = len(want) - len(hip.jpeg_header(150, 40, 95)) - 2
    cap = n - 1000
    buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    scan, length = hip.jpeg_encode(torch.from_numpy(PICTURES["noise150x40"]).to(gpu), out=buf[:cap])
    with pytest.raises(RuntimeError, match=str(n)):
        hip.jpeg_scan(scan, length)
    assert np.all(buf.cpu().numpy()[cap:] == 0xA5)


def avi_chunks(path):
    """The frame chunks of an AVI file, as written."""
    from storage.avi_reader import AviReader
    rd, out = AviReader(path), []
    while True:
        at = rd._next_chunk()
        if at is None:
            return out
        rd._f.seek(at[0])
        out.append(rd._f.read(at[1]))


def assert_chunks_are_the_oracle_files(mjpg_path, plain_path, frames, size):
    from storage.avi_reader import probe, read_frames
    assert probe(mjpg_path) == {**probe(plain_path), "codec": "MJPG"}
    info = probe(mjpg_path)
    assert (info["frames"], info["width"], info["height"]) == (frames, size[0], size[1])
    plain = read_frames(plain_path)                # RGB, what the composer wrote
    chunks = avi_chunks(mjpg_path)
    assert len(chunks) == len(plain) == frames
    for k, (chunk, frame) in enumerate(zip(chunks, plain)):
        assert chunk == jo.encode(frame, 95), f"frame {k}"


@pytest.fixture()
def workdir(tmp_path, monkeypatch):
    from vfml import get_cfg
    from vfml.weights import write_seeded_checkpoint
    write_seeded_checkpoint(str(tmp_path), get_cfg(), seed=0)
    monkeypatch.chdir(tmp_path)
    return tmp_path


def _run(main, argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = main(argv)
    assert rc == 0, out.getvalue()
    return out.getvalue()


def test_flow_processor_writes_the_oracle_mjpg(gpu, workdir, monkeypatch):
    import flow_processor as fp
    from storage import avi_writer
    monkeypatch.setattr(avi_writer, "_pillow", lambda: None)       # the device path's MJPG does not need Pillow
    base = ["--input", "synthetic:160x128x5", "--sequence-length", "3", "--taa", "--device", "cuda"]
    a, b = workdir / "mjpg", workdir / "plain"
    a.mkdir()
    b.mkdir()
    log = _run(fp.main, base + ["--output", str(a)])
    assert "Using MJPG codec" in log and "uncompressed frames instead" not in log
    (cache,) = [p for p in a.iterdir() if p.is_dir()]
    _run(fp.main, base + ["--output", str(b), "--uncompressed", "--use-flow-cache", str(cache)])
    (mjpg,) = [p for p in a.iterdir() if p.suffix == ".avi"]
    (plain,) = [p for p in b.iterdir() if p.suffix == ".avi"]
    assert "MJPG" in mjpg.name
    assert_chunks_are_the_oracle_files(str(mjpg), str(plain), 5, (320, 256))


def test_qa_video_writes_the_oracle_mjpg(gpu, tmp_path):
    import flow_maps
    from storage.cache_manager import FlowCacheManager
    from vfml.synth import synthetic_clip
    h, w, n = 40, 56, 4
    rng = np.random.default_rng(11)
    np.save(tmp_path / "clip.npy", np.stack(synthetic_clip(n, h, w)))
    for i in range(n):
        FlowCacheManager().save_flow_to_cache(rng.normal(0, 2, (h, w, 2)).astype(np.float32), str(tmp_path / "cache"), i,
                                              "npz")
    base = ["--input", str(tmp_path / "clip.npy"), "--flow-cache", str(tmp_path / "cache"), "--kernel-size", "9"]
    _run(flow_maps.main, base + ["--output", str(tmp_path / "mjpg.avi")])
    _run(flow_maps.main, base + ["--output", str(tmp_path / "plain.avi"), "--uncompressed"])
    assert_chunks_are_the_oracle_files(str(tmp_path / "mjpg.avi"), str(tmp_path / "plain.avi"), n - 1, (2 * w, 2 * h))
