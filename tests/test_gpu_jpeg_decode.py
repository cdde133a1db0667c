"""vfml_jpeg_decode_rgb on the MI355X against the numpy restatement (tests/jpeg_decode_oracle.py) and against Pillow,
byte for byte: every file of test_jpeg_decode_cpu.py, row windows into a slice of a larger buffer, the damaged streams
(status cell and guard bytes), the encoder / decoder round trip on the device, --flow-input from an MJPG flow video end
to end and avi_reader.read_frames on the device."""
import contextlib
import ctypes
import functools
import io
import os

import numpy as np
import pytest
import torch

import jpeg_decode_oracle as jd
import jpeg_oracle as jo
from storage import jpeg_parse as jp
from test_jpeg_decode_cpu import PICTURES, WINDOWS, all_files, damaged_files, oracle_decode, pillow_decode

pytestmark = pytest.mark.gpu

FILES = all_files()


def device_decode(gpu, data, **kw):
    from vfml import hip
    rgb, status = hip.jpeg_decode(data, device=gpu, **kw)
    assert status.dtype == torch.int32 and status.is_cuda and int(status.item()) == 0
    hip.jpeg_decode_check(status)
    return rgb.cpu().numpy()


@pytest.mark.parametrize("name", list(FILES))
def test_picture_equals_the_oracle_and_pillow(gpu, name):
    got = device_decode(gpu, FILES[name])
    want = oracle_decode(name)[0]
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ from the oracle"
    assert np.array_equal(got, pillow_decode(FILES[name]))


@functools.lru_cache(maxsize=None)
def wide_file():
    """24 x 1300 noise: 82 MCUs per interval - an interval of many staging steps, a row wider than one workgroup of
    the colour pass."""
    return jo.encode(np.random.default_rng(17).integers(0, 256, (24, 1300, 3), dtype=np.uint8), 95)


def test_long_intervals_and_wide_rows(gpu):
    data = wide_file()
    info = jp.parse(data)
    assert info.restart_interval == 82 and (info.scan[1] - info.scan[0]) // info.intervals > 8 * 1024
    got = device_decode(gpu, data)
    assert np.array_equal(got, pillow_decode(data))
    assert np.array_equal(got, jd.decode(data))
    assert np.array_equal(device_decode(gpu, data, rows=(16, 24)), got[16:24])


def test_a_file_without_restart_markers_is_one_interval(gpu):
    data = FILES["pillow_noise150x40_norst_q95"]
    assert jp.parse(data).restart_interval == 0 and jp.parse(data).intervals == 1
    assert np.array_equal(device_decode(gpu, data), pillow_decode(data))


def test_file_bytes_in_a_pinned_or_device_tensor(gpu):
    from vfml import hip
    data = FILES["random45x67_q95"]
    info = jp.parse(data)
    want = oracle_decode("random45x67_q95")[0]
    host = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    for t in (host.pin_memory(), host.to(gpu)):
        assert np.array_equal(device_decode(gpu, t, info=info), want)
    with pytest.raises(ValueError):
        hip.jpeg_decode(host, info=info, device=gpu)          # pageable host memory
    with pytest.raises(ValueError):
        hip.jpeg_decode(host.to(gpu))                         # no header information
    with pytest.raises(jp.JpegUnsupported, match="progressive"):
        hip.jpeg_decode(data.replace(b'\xff\xc0', b'\xff\xc2', 1), device=gpu)


@pytest.mark.parametrize("rows", WINDOWS)
@pytest.mark.parametrize("name", ["noise150x40_q95", "pillow_noise150x40_rows1_q60", "pillow_noise150x40_norst_q95"])
def test_row_window_into_a_slice_of_a_larger_buffer(gpu, name, rows):
    y0, y1 = rows
    h, w = 150, 40
    big = torch.full((y1 - y0 + 8, w + 13, 3), 0xA5, dtype=torch.uint8, device=gpu)
    view = big[3:3 + y1 - y0, :w]                  # row stride 3 (w + 13) > 3 w, an odd row offset
    assert view.stride(0) == 3 * (w + 13)
    device_decode(gpu, FILES[name], rows=rows, out=view)
    host = big.cpu().numpy()
    assert np.array_equal(host[3:3 + y1 - y0, :w], oracle_decode(name)[0][y0:y1])
    host[3:3 + y1 - y0, :w] = 0xA5
    assert np.all(host == 0xA5)


def test_row_window_with_intervals_that_are_no_mcu_rows(gpu):
    name = "pillow_random45x67_blocks3_opt_q85"
    assert np.array_equal(device_decode(gpu, FILES[name], rows=(20, 45)), oracle_decode(name)[0][20:45])


@pytest.mark.parametrize("name", ["half_32x32", "rst_removed_150x40", "zeros_150x40"])
def test_damaged_streams_end_in_the_status_cell(gpu, name):
    """The kernels' clamps: the entry point is called with a workspace and an output that carry guard bytes."""
    from vfml import hip
    data = damaged_files()[name]
    with pytest.raises(jd.JpegError):
        jd.decode(data)
    info = jp.parse(data)
    h, w = info.h, info.w
    L = hip.lib()
    scan_host = torch.frombuffer(bytearray(data[info.scan[0]:info.scan[1]]), dtype=torch.uint8)
    guard = 4096
    scan = torch.full((scan_host.numel() + guard,), 0xFF, dtype=torch.uint8, device=gpu)       # FFs behind the scan
    scan[:scan_host.numel()] = scan_host.to(gpu)
    need = int(L.vfml_jpeg_decode_workspace_bytes(h, w, scan_host.numel()))
    assert need > 0
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    out = torch.full((guard + 3 * h * w + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    qt, tables = (torch.from_numpy(t.reshape(-1).copy()).to(gpu) for t in jp.decode_tables(info))
    status = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rc = L.vfml_jpeg_decode_rgb(p(scan), scan_host.numel(), h, w, info.restart_interval, p(qt), p(tables), 0, h, p(ws),
                                p(out, guard), 3 * w, p(status), None)
    assert rc == 0, L.vfml_last_error()
    torch.cuda.synchronize()
    assert int(status.item()) not in (0, -1)
    with pytest.raises(RuntimeError, match="damaged scan"):
        hip.jpeg_decode_check(status)
    assert bool((ws[need:] == 0xA5).all()) and bool((out[:guard] == 0xA5).all())
    assert bool((out[guard + 3 * h * w:] == 0xA5).all())
    # and through the library call
    _, status = hip.jpeg_decode(data, device=gpu)
    with pytest.raises(RuntimeError, match="damaged scan"):
        hip.jpeg_decode_check(status)


def test_rejected_arguments_launch_nothing(gpu):
    from vfml import hip
    L = hip.lib()
    assert L.vfml_jpeg_decode_workspace_bytes(0, 8, 10) == 0 and L.vfml_jpeg_decode_workspace_bytes(8, 8, 1 << 31) == 0
    assert L.vfml_jpeg_decode_workspace_bytes(16, 16, 0) > 0
    t = torch.zeros(8192, dtype=torch.uint8, device=gpu)
    p = ctypes.c_void_p(t.data_ptr())
    assert L.vfml_jpeg_decode_rgb(p, 10, 8, 8, 0, p, p, 0, 9, p, p, 24, p, None) != 0 and b"rows" in L.vfml_last_error()
    assert L.vfml_jpeg_decode_rgb(p, 10, 8, 8, 0, p, p, 0, 8, p, p, 23, p, None) != 0 and b"stride" in L.vfml_last_error()
    assert L.vfml_jpeg_decode_rgb(None, 10, 8, 8, 0, p, p, 0, 8, p, p, 24, p, None) != 0
    with pytest.raises(ValueError):
        hip.jpeg_decode(FILES["one1x1_q95"], rows=(0, 2), device=gpu)


@pytest.mark.parametrize("name", ["random45x67", "noise150x40", "frequency150x40"])
def test_encoder_decoder_round_trip_on_the_device(gpu, name):
    from vfml import hip
    x = torch.from_numpy(PICTURES[name]).to(gpu)
    h, w = x.shape[:2]
    data = hip.jpeg_file(hip.jpeg_header(h, w, 95), hip.jpeg_scan(*hip.jpeg_encode(x)))
    assert np.array_equal(device_decode(gpu, data), pillow_decode(data))


# ---- the readers -----------------------------------------------------------------------------------------------------
def _run(main, argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = main(argv)
    assert rc == 0, out.getvalue()
    return out.getvalue()


def _only(directory, suffix):
    (path,) = [p for p in directory.iterdir() if p.suffix == suffix]
    return path


@pytest.fixture(scope="module")
def flow_job(gpu, tmp_path_factory):
    """Rendered once for the tests below: a directory with the seeded checkpoint, an MJPG flow video (original over
    motion-vectors-rg8 picture) written there by the device encoder, and its cache."""
    import flow_processor as fp
    from vfml import get_cfg
    from vfml.weights import write_seeded_checkpoint
    work = tmp_path_factory.mktemp("flow_job")
    write_seeded_checkpoint(str(work), get_cfg(), seed=0)
    out = work / "flowvideo"
    out.mkdir()
    cwd = os.getcwd()
    os.chdir(work)
    try:
        _run(fp.main, ["--input", "synthetic:160x128x5", "--sequence-length", "3", "--flow-only", "--flow-format",
                       "motion-vectors-rg8", "--device", "cuda", "--output", str(out)])
    finally:
        os.chdir(cwd)
    (cache,) = [p for p in out.iterdir() if p.is_dir()]
    return work, _only(out, ".avi"), cache


def test_flow_input_from_an_mjpg_flow_video(gpu, flow_job, tmp_path, monkeypatch):
    import flow_processor as fp
    from storage import avi_reader
    work, mjpg, cache = flow_job
    monkeypatch.chdir(work)
    workdir = tmp_path
    assert avi_reader.probe(str(mjpg)) == {"frames": 5, "fps": avi_reader.probe(str(mjpg))["fps"], "width": 160,
                                           "height": 256, "codec": "MJPG"}
    stack = workdir / "flowvideo.npy"
    np.save(stack, np.stack(avi_reader.read_frames(str(mjpg))))           # the frames as Pillow decodes them

    def job(name, flow_input):
        out = workdir / name
        out.mkdir()
        _run(fp.main, ["--input", "synthetic:160x128x5", "--sequence-length", "3", "--taa", "--flow-format",
                       "motion-vectors-rg8", "--device", "cuda", "--uncompressed", "--use-flow-cache", str(cache),
                       "--flow-input", str(flow_input), "--output", str(out)])
        return _only(out, ".avi").read_bytes()

    from_npy = job("npy", stack)
    as_is = job("avi", mjpg)
    monkeypatch.setattr(avi_reader, "_pillow", lambda: None)              # the device path does not need Pillow
    without_pillow = job("nopillow", mjpg)
    assert len(as_is) > 5 * 3 * 128 * 2 * 160 * 3
    assert as_is == without_pillow
    assert as_is == from_npy


def test_read_frames_on_the_device(gpu, flow_job, tmp_path, monkeypatch):
    from storage import avi_reader
    from storage.avi_writer import AviWriter
    mjpg = str(flow_job[1])
    want = avi_reader.read_frames(mjpg)
    ri0 = str(tmp_path / "pillow.avi")                # Pillow's files have no restart intervals: the fallback
    wr = AviWriter(ri0, 'MJPG', 25.0, (67, 45))
    for k in range(3):
        wr.write(np.roll(PICTURES["random45x67"], 5 * k, axis=1))
    wr.release()
    want0 = avi_reader.read_frames(ri0)
    got0 = avi_reader.read_frames(ri0, device=gpu)
    assert len(got0) == len(want0) == 3 and all(np.array_equal(a, b) for a, b in zip(got0, want0))
    monkeypatch.setattr(avi_reader, "_pillow", lambda: None)
    got = avi_reader.read_frames(mjpg, device=gpu)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.dtype == np.uint8 and a.shape == (256, 160, 3) and np.array_equal(a, b)
    part = avi_reader.read_frames(mjpg, 1, 2, device=gpu)
    assert len(part) == 2 and np.array_equal(part[0], want[1]) and np.array_equal(part[1], want[2])
