"""vfml_jpeg_decode_rgb_sync on the MI355X: the self-synchronising decoder against Pillow and
the numpy oracle byte for byte on files without restart markers and with every other kind of interval, chains of
subsequences across workgroups (with speculation that agrees late and never), both kernels against each other, row
windows into a slice of a larger buffer, the damaged streams (status cell and guard bytes), rejected arguments, and the
readers that now hand frames without restart intervals to the device."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import jpeg_decode_oracle as jd
from storage import jpeg_parse as jp
from test_gpu_jpeg_decode import _only, _run, flow_job  # noqa: F401  (flow_job: the module fixture, made here once more)
from test_jpeg_decode_cpu import PICTURES, own_file, pillow_decode, pillow_file
from test_jpeg_selfsync_cpu import DAMAGED, FILES, FLIP_BITS, damaged, serial_error_bit

pytestmark = pytest.mark.gpu

GPU_SIZES = (16, 128)


def device_decode(gpu, data, **kw):
    from vfml import hip
    rgb, status = hip.jpeg_decode(data, device=gpu, **kw)
    assert status.dtype == torch.int32 and status.is_cuda and int(status.item()) == 0
    return rgb.cpu().numpy()


@functools.lru_cache(maxsize=None)
def references(name):
    data = FILES[name]
    return jd.decode(data), pillow_decode(data)


@pytest.mark.parametrize("S", GPU_SIZES)
@pytest.mark.parametrize("name", list(FILES))
def test_the_matrix(gpu, name, S):
    oracle, pillow = references(name)
    got = device_decode(gpu, FILES[name], plan="sync", subseq_bytes=S)
    assert got.shape == pillow.shape and got.dtype == np.uint8
    assert np.array_equal(got, pillow), f"{(got != pillow).sum()} bytes differ from Pillow"
    assert np.array_equal(got, oracle)


@functools.lru_cache(maxsize=None)
def large_files():
    """208 x 240 pictures without restart markers: noise at quality 100 (the picture of test_gpu_mjpg_reader; a scan
    above 64 KiB, more than 4096 subsequences of 16 bytes) and the checkerboard, on which speculation never agrees."""
    noise = np.random.default_rng(5).integers(0, 256, (208, 240, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:208, 0:240]
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    return {"noise": pillow_file(noise, quality=100), "checker": pillow_file(checker, quality=95)}


@pytest.mark.parametrize("name", ["noise", "checker"])
def test_chains_across_workgroups(gpu, name):
    data = large_files()[name]
    info = jp.parse(data)
    n = info.scan[1] - info.scan[0]
    assert info.restart_interval == 0
    assert n > (1 << 16 if name == "noise" else 3 * 256 * 16)           # several groups of 256 subsequences
    want = pillow_decode(data)
    assert np.array_equal(device_decode(gpu, data, plan="sync", subseq_bytes=16), want)
    assert np.array_equal(device_decode(gpu, data, plan="sync"), want)


@pytest.mark.parametrize("name", ["norst_noise150x40_q95", "own_noise150x40_q95", "wide_ri82"])
def test_both_plans_agree(gpu, name):
    from vfml import hip
    data = FILES[name]
    a = device_decode(gpu, data, plan="sync")
    b = device_decode(gpu, data, plan="interval")
    assert np.array_equal(a, b) and np.array_equal(a, references(name)[1])
    want = {"norst_noise150x40_q95": "sync", "own_noise150x40_q95": "interval", "wide_ri82": "interval"}[name]
    assert hip.jpeg_decode_plan(jp.parse(data)) == want
    assert np.array_equal(device_decode(gpu, data), a)
    with pytest.raises(ValueError):
        hip.jpeg_decode(data, device=gpu, plan="serial")
    with pytest.raises(ValueError):
        hip.jpeg_decode(data, device=gpu, plan="sync", subseq_bytes=24)


@pytest.mark.parametrize("rows", [(75, 150), (37, 90), (149, 150)])
def test_row_window_into_a_slice_of_a_larger_buffer(gpu, rows):
    name = "norst_noise150x40_q95"
    y0, y1 = rows
    h, w = 150, 40
    big = torch.full((y1 - y0 + 8, w + 13, 3), 0xA5, dtype=torch.uint8, device=gpu)
    view = big[3:3 + y1 - y0, :w]
    device_decode(gpu, FILES[name], rows=rows, out=view, plan="sync", subseq_bytes=32)
    host = big.cpu().numpy()
    assert np.array_equal(host[3:3 + y1 - y0, :w], references(name)[1][y0:y1])
    host[3:3 + y1 - y0, :w] = 0xA5
    assert np.all(host == 0xA5)


@pytest.mark.parametrize("S", GPU_SIZES)
@pytest.mark.parametrize("name", DAMAGED)
def test_damaged_streams_end_in_the_status_cell(gpu, name, S):
    """Defined results on fixed files: the entry point is called with a workspace and an output that carry guard bytes."""
    from vfml import hip
    data = damaged(name)
    bit = serial_error_bit(data)
    assert bit == FLIP_BITS.get(name, bit)
    info = jp.parse(data)
    h, w = info.h, info.w
    L = hip.lib()
    scan_host = torch.frombuffer(bytearray(data[info.scan[0]:info.scan[1]]), dtype=torch.uint8)
    guard = 4096
    scan = torch.full((scan_host.numel() + guard,), 0xFF, dtype=torch.uint8, device=gpu)       # FFs behind the scan
    scan[:scan_host.numel()] = scan_host.to(gpu)
    need = int(L.vfml_jpeg_decode_sync_workspace_bytes(h, w, scan_host.numel(), S))
    assert need > int(L.vfml_jpeg_decode_workspace_bytes(h, w, scan_host.numel())) > 0
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    out = torch.full((guard + 3 * h * w + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    qt, tables = (torch.from_numpy(t.reshape(-1).copy()).to(gpu) for t in jp.decode_tables(info))
    status = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rc = L.vfml_jpeg_decode_rgb_sync(p(scan), scan_host.numel(), h, w, info.restart_interval, p(qt), p(tables), 0, h, S,
                                     p(ws), p(out, guard), 3 * w, p(status), None)
    assert rc == 0, L.vfml_last_error()
    torch.cuda.synchronize()
    got = int(status.item())
    assert got not in (0, -1) and got & bit, (got, bit)
    with pytest.raises(RuntimeError, match="damaged scan"):
        hip.jpeg_decode_check(status)
    assert bool((ws[need:] == 0xA5).all()) and bool((out[:guard] == 0xA5).all())
    assert bool((out[guard + 3 * h * w:] == 0xA5).all())


def test_rejected_arguments_launch_nothing(gpu):
    from vfml import hip
    L = hip.lib()
    size = L.vfml_jpeg_decode_sync_workspace_bytes
    assert size(8, 8, 1 << 31, 128) == 0 and size(0, 8, 10, 128) == 0
    for S in (0, 24, 2048):
        assert size(8, 8, 10, S) == 0
    assert size(16, 16, 0, 16) > 0
    t = torch.full((8192,), 0xA5, dtype=torch.uint8, device=gpu)
    p = ctypes.c_void_p(t.data_ptr())
    call = L.vfml_jpeg_decode_rgb_sync
    for S in (0, 24, 2048):
        assert call(p, 10, 8, 8, 0, p, p, 0, 8, S, p, p, 24, p, None) != 0 and b"subsequences" in L.vfml_last_error()
    assert call(p, 10, 8, 8, 0, p, p, 0, 8, 128, ctypes.c_void_p(t.data_ptr() + 64), p, 24, p, None) != 0
    assert b"aligned" in L.vfml_last_error()
    assert call(p, 1 << 31, 8, 8, 0, p, p, 0, 8, 128, p, p, 24, p, None) != 0 and b"2 GiB" in L.vfml_last_error()
    assert call(p, 10, 8, 8, 0, p, p, 0, 9, 128, p, p, 24, p, None) != 0 and b"rows" in L.vfml_last_error()
    torch.cuda.synchronize()
    assert bool((t == 0xA5).all())


# ---- the readers -----------------------------------------------------------------------------------------------------
def test_read_frames_of_frames_without_restart_intervals(gpu, tmp_path, monkeypatch):
    from storage import avi_reader
    from storage.avi_writer import AviWriter
    path = str(tmp_path / "pillow.avi")
    wr = AviWriter(path, 'MJPG', 25.0, (67, 45))                       # the host writer: Pillow's files, no DRI
    for k in range(3):
        wr.write(np.roll(PICTURES["random45x67"], 5 * k, axis=1))
    wr.release()
    with avi_reader.AviReader(path) as r:
        assert jp.parse(r.read_chunk()).restart_interval == 0
    want = avi_reader.read_frames(path)
    monkeypatch.setattr(avi_reader, "_pillow", lambda: None)            # the device path does not need Pillow
    got = avi_reader.read_frames(path, device=gpu)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert a.dtype == np.uint8 and a.shape == (45, 67, 3) and np.array_equal(a, b)


def test_the_decoder_counts_frames_per_plan(gpu):
    from storage.device_mjpg import DeviceMjpgDecoder
    files = [FILES["norst_random45x67_q95"], own_file("random45x67", 95), FILES["norst_random45x67_q75"]]
    dec = DeviceMjpgDecoder(gpu)
    assert dec.stats == {"interval": 0, "sync": 0}
    with torch.cuda.device(gpu):
        got = [dec.submit(f).cpu().numpy() for f in files]
        got.append(dec.submit(files[1], plan="sync", subseq_bytes=64).cpu().numpy())
        got.append(dec.submit(files[1], subseq_bytes=64).cpu().numpy())     # the rule says 'interval': the size is unused
        with pytest.raises(ValueError):
            dec.submit(files[1], plan="interval", subseq_bytes=64)
        dec.finish()
    assert dec.stats == {"interval": 2, "sync": 3}
    for g, f in zip(got, files + [files[1], files[1]]):
        assert np.array_equal(g, pillow_decode(f))


def test_flow_input_from_a_flow_video_without_restart_intervals(gpu, flow_job, tmp_path, monkeypatch):
    """The flow video as the reference's writer leaves it - MJPG frames without a DRI segment - decoded on the device:
    the output equals the .npy route (the frames as Pillow decodes them) byte for byte, without Pillow in the job."""
    import flow_processor as fp
    from storage import avi_reader, device_mjpg
    from storage.avi_writer import AviWriter
    work, mjpg, cache = flow_job
    monkeypatch.chdir(work)
    ri0 = str(tmp_path / "flow_ri0.avi")
    wr = AviWriter(ri0, 'MJPG', 25.0, (160, 256))
    for frame in avi_reader.read_frames(str(mjpg)):
        wr.write(frame)
    wr.release()
    with avi_reader.AviReader(ri0) as r:
        assert jp.parse(r.read_chunk()).restart_interval == 0
    stack = tmp_path / "flowvideo.npy"
    np.save(stack, np.stack(avi_reader.read_frames(ri0)))
    seen = []
    submit = device_mjpg.DeviceMjpgDecoder.submit

    def counted(self, *a, **kw):
        out = submit(self, *a, **kw)
        seen.append(dict(self.stats))
        return out

    monkeypatch.setattr(device_mjpg.DeviceMjpgDecoder, "submit", counted)

    def job(name, flow_input):
        out = tmp_path / name
        out.mkdir()
        _run(fp.main, ["--input", "synthetic:160x128x5", "--sequence-length", "3", "--taa", "--flow-format",
                       "motion-vectors-rg8", "--device", "cuda", "--uncompressed", "--use-flow-cache", str(cache),
                       "--flow-input", str(flow_input), "--output", str(out)])
        return _only(out, ".avi").read_bytes()

    from_npy = job("npy", stack)
    assert not seen
    monkeypatch.setattr(avi_reader, "_pillow", lambda: None)
    as_is = job("avi", ri0)
    assert seen and seen[-1] == {"interval": 0, "sync": 5}
    assert len(as_is) > 5 * 3 * 128 * 2 * 160 * 3
    assert as_is == from_npy
