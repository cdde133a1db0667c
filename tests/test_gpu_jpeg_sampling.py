"""vfml_jpeg_decode_rgb_sampled and vfml_jpeg_decode_rgb_sync_sampled on the MI355X for 4:4:4, 4:2:2 and grey files,
byte for byte against Pillow and the numpy definition (tests/jpeg_sampling_oracle.py): the files of
test_jpeg_sampling_cpu.py through both kernels, a scan of more than one wave of subsequences, the --flow-input row window
into a slice of a larger buffer, the damaged files (status cell, guard bytes, the next decode on the same workspace), an
MJPG stream that mixes the samplings, and --flow-input from a 4:4:4 flow video end to end."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import jpeg_oracle as jo
import jpeg_sampling_oracle as so
from storage import jpeg_parse as jp
from test_jpeg_sampling_cpu import (SAMPLING_CODE, SAMPLINGS, SIZES, Image, damaged_files, picture, pillow_decode,
                                    pillow_file)

pytestmark = pytest.mark.gpu


def device_decode(gpu, data, **kw):
    from vfml import hip
    rgb, status = hip.jpeg_decode(data, device=gpu, **kw)
    assert int(status.item()) == 0
    return rgb.cpu().numpy()


def _equal(got, data, what):
    want = pillow_decode(data)
    assert got.shape == want.shape and got.dtype == np.uint8, what
    assert np.array_equal(got, want), f"{what}: {(got != want).sum()} bytes differ from Pillow"
    assert np.array_equal(got, so.decode(data)), what


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_interval_plan_equals_pillow_and_the_oracle(gpu, sampling, size):
    """One MCU row per interval: a wave per interval."""
    for kind, q in (("random", 95), ("smooth", 30)):
        data = pillow_file(sampling, kind, *size, "rows1", q)
        assert jp.decode_plan(jp.parse(data, jp.DEVICE_SAMPLINGS)) == "interval"
        _equal(device_decode(gpu, data, plan="interval"), data, (kind, q))
        _equal(device_decode(gpu, data), data, (kind, q, "by the rule"))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_sync_plan_equals_pillow_and_the_oracle(gpu, sampling, size):
    """No markers and 3 MCUs per interval, a lane per 16 and per 128 bytes of the scan."""
    for restart in ("norst", "blocks3"):
        for kind, q in (("random", 95), ("smooth", 30)):
            data = pillow_file(sampling, kind, *size, restart, q)
            for S in (16, 128):
                _equal(device_decode(gpu, data, plan="sync", subseq_bytes=S), data, (restart, kind, q, S))


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_more_than_one_wave_of_subsequences(gpu, sampling):
    data = pillow_file(sampling, "random", 208, 240, "norst", 95)
    info = jp.parse(data, jp.DEVICE_SAMPLINGS)
    assert info.restart_interval == 0 and (info.scan[1] - info.scan[0]) // 128 > 2 * 64
    _equal(device_decode(gpu, data), data, "by the rule")
    _equal(device_decode(gpu, data, plan="sync", subseq_bytes=16), data, 16)
    _equal(device_decode(gpu, data, plan="interval"), data, "one interval")


def test_marker_numbers_wrap(gpu):
    data = pillow_file("4:4:4", "random", 40, 150, "blocks3", 95)
    assert jp.parse(data, jp.DEVICE_SAMPLINGS).intervals == 32
    for plan in ("interval", "sync"):
        _equal(device_decode(gpu, data, plan=plan), data, plan)


@pytest.mark.parametrize("restart", ("rows1", "norst"))
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_flow_input_window_into_a_slice_of_a_larger_buffer(gpu, sampling, restart):
    h, w = 45, 67
    y0, y1 = h // 2, h
    data = pillow_file(sampling, "random", h, w, restart, 95)
    big = torch.full((y1 - y0 + 8, w + 13, 3), 0xA5, dtype=torch.uint8, device=gpu)
    view = big[3:3 + y1 - y0, :w]
    device_decode(gpu, data, rows=(y0, y1), out=view)
    host = big.cpu().numpy()
    assert np.array_equal(host[3:3 + y1 - y0, :w], pillow_decode(data)[y0:y1])
    host[3:3 + y1 - y0, :w] = 0xA5
    assert np.all(host == 0xA5)


@pytest.mark.parametrize("sync", (False, True), ids=("interval", "sync"))
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_damaged_files_end_in_the_status_cell(gpu, sampling, sync):
    """Workspace and output carry guard bytes; the whole file of the same size is then decoded on the same workspace."""
    from vfml import hip
    L = hip.lib()
    good = pillow_file(sampling, "random", 17, 33, "rows1", 95)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    guard, S = 4096, 16
    h, w = 17, 33
    samp = SAMPLING_CODE[sampling]
    cap = max(len(f) for f in (good, *damaged_files(sampling).values()))
    need = int(L.vfml_jpeg_decode_sync_sampled_workspace_bytes(h, w, samp, cap, S) if sync else
               L.vfml_jpeg_decode_sampled_workspace_bytes(h, w, samp, cap))
    assert need > 0
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    out = torch.full((guard + 3 * h * w + guard,), 0xA5, dtype=torch.uint8, device=gpu)

    def run(data):
        info = jp.parse(data, jp.DEVICE_SAMPLINGS)
        assert (info.h, info.w, info.sampling) == (h, w, sampling)
        raw = torch.frombuffer(bytearray(data[info.scan[0]:info.scan[1]]), dtype=torch.uint8)
        scan = torch.full((raw.numel() + guard,), 0xFF, dtype=torch.uint8, device=gpu)        # FFs behind the scan
        scan[:raw.numel()] = raw.to(gpu)
        qt, tables = (torch.from_numpy(t.reshape(-1).copy()).to(gpu) for t in jp.decode_tables(info))
        status = torch.full((1,), -1, dtype=torch.int32, device=gpu)
        head = (p(scan), raw.numel(), h, w, samp, info.restart_interval, p(qt), p(tables), 0, h)
        tail = (p(ws), p(out, guard), 3 * w, p(status), None)
        rc = L.vfml_jpeg_decode_rgb_sync_sampled(*head, S, *tail) if sync else L.vfml_jpeg_decode_rgb_sampled(*head, *tail)
        assert rc == 0, L.vfml_last_error()
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()) and bool((out[:guard] == 0xA5).all())
        assert bool((out[guard + 3 * h * w:] == 0xA5).all())
        return int(status.item())

    for name, data in damaged_files(sampling).items():
        with pytest.raises(so.JpegError):
            so.decode(data)
        status = run(data)
        assert status not in (0, -1), name
        with pytest.raises(RuntimeError, match="damaged scan"):
            hip.jpeg_decode_check(status)
        assert run(good) == 0
        got = out[guard:guard + 3 * h * w].cpu().numpy().reshape(h, w, 3)
        assert np.array_equal(got, pillow_decode(good)), name


def test_rejected_arguments_launch_nothing(gpu):
    from vfml import hip
    L = hip.lib()
    t = torch.zeros(8192, dtype=torch.uint8, device=gpu)
    p = ctypes.c_void_p(t.data_ptr())
    for samp in (-1, 4):
        assert L.vfml_jpeg_decode_sampled_workspace_bytes(8, 8, samp, 10) == 0
        assert L.vfml_jpeg_decode_sync_sampled_workspace_bytes(8, 8, samp, 10, 128) == 0
        assert L.vfml_jpeg_decode_rgb_sampled(p, 10, 8, 8, samp, 0, p, p, 0, 8, p, p, 24, p, None) != 0
        assert b"sampling" in L.vfml_last_error()
        assert L.vfml_jpeg_decode_rgb_sync_sampled(p, 10, 8, 8, samp, 0, p, p, 0, 8, 128, p, p, 24, p, None) != 0
        assert b"sampling" in L.vfml_last_error()
    assert L.vfml_jpeg_decode_rgb_sampled(p, 10, 8, 8, 3, 0, p, p, 0, 9, p, p, 24, p, None) != 0 and b"rows" in L.vfml_last_error()
    assert L.vfml_jpeg_decode_rgb_sync_sampled(p, 10, 8, 8, 1, 0, p, p, 0, 8, 24, p, p, 24, p, None) != 0
    assert b"subsequences" in L.vfml_last_error()
    # the samplings size their own workspaces: 4:4:4 holds twice the coefficients of 4:2:0, grey no chroma planes
    sizes = [L.vfml_jpeg_decode_sampled_workspace_bytes(64, 64, s, 4096) for s in range(4)]
    assert sizes[0] == L.vfml_jpeg_decode_workspace_bytes(64, 64, 4096)
    assert sizes[3] < sizes[0] < sizes[1] < sizes[2]


# ---- the readers -----------------------------------------------------------------------------------------------------
def _avi(path, files, size):
    from storage.avi_writer import AviWriter
    wr = AviWriter(str(path), 'MJPG', 25.0, size, encoder='external')
    for f in files:
        wr.write_encoded(f)
    wr.release()
    return str(path)


def test_a_stream_that_mixes_the_samplings(gpu, tmp_path, monkeypatch):
    from storage import avi_reader
    h, w = 45, 67
    img = picture("random", h, w)
    buf = io.BytesIO()
    Image.fromarray(np.roll(img, 9, axis=1), "RGB").save(buf, format="JPEG", quality=90, subsampling="4:2:0")
    files = [jo.encode(img, 95), pillow_file("4:4:4", "random", h, w), pillow_file("4:2:2", "smooth", h, w, "rows1"),
             pillow_file("grey", "random", h, w), b'', buf.getvalue()]
    kinds = [jp.parse(f, jp.DEVICE_SAMPLINGS).sampling for f in files if f]
    assert kinds == ["4:2:0", "4:4:4", "4:2:2", "grey", "4:2:0"] and jp.parse(files[0]).restart_interval > 0
    path = _avi(tmp_path / "mixed.avi", files, (w, h))
    want = avi_reader.read_frames(path)
    assert len(want) == 6 and np.array_equal(want[4], want[3])
    got = avi_reader.read_frames(path, device=gpu)
    monkeypatch.setattr(avi_reader, "_pillow", lambda: None)          # nothing goes to the host
    alone = avi_reader.read_frames(path, device=gpu)
    for frames in (got, alone):
        assert len(frames) == len(want)
        for k, (a, b) in enumerate(zip(frames, want)):
            assert a.dtype == np.uint8 and a.shape == (h, w, 3) and np.array_equal(a, b), f"frame {k}"


def _run(main, argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = main(argv)
    assert rc == 0, out.getvalue()
    return out.getvalue()


def _only(directory, suffix):
    (path,) = [p for p in directory.iterdir() if p.suffix == suffix]
    return path


def test_flow_input_from_a_444_flow_video(gpu, tmp_path, monkeypatch):
    """A flow video rendered here, its frames written again by Pillow as 4:4:4 JPEG files: --flow-input from that .avi,
    with Pillow patched out, renders the bytes it renders from the same pictures given as .npy."""
    import flow_processor as fp
    from storage import avi_reader
    from vfml import get_cfg
    from vfml.weights import write_seeded_checkpoint
    write_seeded_checkpoint(str(tmp_path), get_cfg(), seed=0)
    monkeypatch.chdir(tmp_path)
    first = tmp_path / "flowvideo"
    first.mkdir()
    _run(fp.main, ["--input", "synthetic:160x128x5", "--sequence-length", "3", "--flow-only", "--flow-format",
                   "motion-vectors-rg8", "--device", "cuda", "--output", str(first)])
    (cache,) = [p for p in first.iterdir() if p.is_dir()]
    files = []
    for frame in avi_reader.read_frames(str(_only(first, ".avi"))):
        buf = io.BytesIO()
        Image.fromarray(frame, "RGB").save(buf, format="JPEG", quality=95, subsampling="4:4:4")
        files.append(buf.getvalue())
    assert len(files) == 5 and all(jp.parse(f, jp.DEVICE_SAMPLINGS).sampling == "4:4:4" for f in files)
    video = _avi(tmp_path / "flow444.avi", files, (160, 256))
    stack = tmp_path / "flow444.npy"
    np.save(stack, np.stack([pillow_decode(f) for f in files]))

    def job(name, flow_input):
        out = tmp_path / name
        out.mkdir()
        _run(fp.main, ["--input", "synthetic:160x128x5", "--sequence-length", "3", "--taa", "--flow-format",
                       "motion-vectors-rg8", "--device", "cuda", "--uncompressed", "--use-flow-cache", str(cache),
                       "--flow-input", str(flow_input), "--output", str(out)])
        return _only(out, ".avi").read_bytes()

    from_npy = job("npy", stack)
    monkeypatch.setattr(avi_reader, "_pillow", lambda: None)
    from_avi = job("avi", video)
    assert len(from_avi) > 5 * 3 * 128 * 2 * 160 * 3
    assert from_avi == from_npy
