"""vfml_jpeg_encode_rgb_sampled on the MI355X against the numpy definition (tests/jpeg_encode_sampling_oracle.py), byte for
byte: the pictures of test_jpeg_cpu.py at 4:2:2 and 4:4:4 (odd MCU-row and MCU-column counts, 16 x 16 regions whose second
MCU row or column is outside the grid, the marker wrap), an interval of more than 1024 blocks, 4:2:0 against the entry
point it generalises, strided input, placement in a larger buffer, a capacity that is too small, the device decoder's
round trip, rejected samplings, and flow_processor's MJPG_SAMPLING end to end."""
import contextlib
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import jpeg_encode_sampling_oracle as eo
import jpeg_oracle as jo
from storage import jpeg_parse as jp

pytestmark = pytest.mark.gpu

PICTURES = jo.pictures()
NEW = ("4:2:2", "4:4:4")


@functools.lru_cache(maxsize=None)
def oracle_file(name, sampling):
    return eo.encode(PICTURES[name], 95, sampling)


def gpu_file(hip, img, quality=95, sampling="4:2:0", **kw):
    scan, length = hip.jpeg_encode(img, quality, sampling=sampling, **kw)
    h, w = img.shape[:2]
    return hip.jpeg_file(hip.jpeg_header(h, w, quality, sampling), hip.jpeg_scan(scan, length))


def pillow_decode(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", list(PICTURES))
@pytest.mark.parametrize("sampling", NEW)
def test_stream_equals_the_oracle(gpu, sampling, name):
    from vfml import hip
    got = gpu_file(hip, torch.from_numpy(PICTURES[name]).to(gpu), sampling=sampling)
    want = oracle_file(name, sampling)
    assert len(got) == len(want), (len(got), len(want))
    assert got == want


def test_an_interval_of_more_than_1024_blocks(gpu):
    """8 x 2800 at 4:4:4: 350 MCUs x 3 = 1050 blocks in one interval, the interval kernel's scan takes two passes."""
    from vfml import hip
    img = np.random.default_rng(8).integers(0, 256, (8, 2800, 3), dtype=np.uint8)
    assert gpu_file(hip, torch.from_numpy(img).to(gpu), sampling="4:4:4") == eo.encode(img, 95, "4:4:4")


def old_entry_point(hip, img, quality):
    """The scan vfml_jpeg_encode_rgb itself writes (hip.jpeg_encode goes through the sampled entry point)."""
    from storage import jpeg_tables
    L = hip.lib()
    h, w = img.shape[:2]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = torch.empty(int(L.vfml_jpeg_workspace_bytes(h, w)), dtype=torch.uint8, device=img.device)
    qt = torch.from_numpy(jpeg_tables.quant_tables(quality).copy()).to(img.device)
    scan = torch.empty(int(L.vfml_jpeg_scan_capacity(h, w)), dtype=torch.uint8, device=img.device)
    length = torch.zeros(1, dtype=torch.int32, device=img.device)
    rc = L.vfml_jpeg_encode_rgb(p(img), h, w, 3 * w, p(qt), p(ws), p(scan), scan.numel(), p(length),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.vfml_last_error()
    return hip.jpeg_scan(scan, length)


@pytest.mark.parametrize("quality", [50, 95, 100])
def test_420_is_the_entry_point_it_generalises(gpu, quality):
    from vfml import hip
    L = hip.lib()
    for name in ("random45x67", "noise150x40"):
        img = PICTURES[name]
        h, w = img.shape[:2]
        dev = torch.from_numpy(img).to(gpu)
        new = gpu_file(hip, dev, quality, "4:2:0")
        assert new == jo.encode(img, quality)
        assert new == gpu_file(hip, dev, quality)                       # the default
        assert hip.jpeg_file(hip.jpeg_header(h, w, quality), old_entry_point(hip, dev, quality)) == new
        assert L.vfml_jpeg_sampled_workspace_bytes(h, w, 0) == L.vfml_jpeg_workspace_bytes(h, w) > 0
        assert L.vfml_jpeg_sampled_scan_capacity(h, w, 0) == L.vfml_jpeg_scan_capacity(h, w) > 0


def test_row_slice_of_a_larger_buffer(gpu):
    from vfml import hip
    img = PICTURES["random45x67"]
    h, w = img.shape[:2]
    big = torch.full((h + 8, w + 13, 3), 201, dtype=torch.uint8, device=gpu)
    big[3:3 + h, :w] = torch.from_numpy(img).to(gpu)
    view = big[3:3 + h, :w]                        # row stride 3 (w + 13) > 3 w, an odd row offset
    assert view.stride(0) == 3 * (w + 13) and not view.is_contiguous()
    for sampling in NEW:
        assert gpu_file(hip, view, sampling=sampling) == oracle_file("random45x67", sampling)


def test_out_inside_a_larger_buffer(gpu):
    from vfml import hip
    want = oracle_file("noise150x40", "4:4:4")
    header = hip.jpeg_header(150, 40, 95, "4:4:4")
    n = len(want) - len(header) - 2
    buf = torch.full((n + 64 + 37,), 0xA5, dtype=torch.uint8, device=gpu)
    scan, length = hip.jpeg_encode(torch.from_numpy(PICTURES["noise150x40"]).to(gpu), out=buf[37:37 + n + 5],
                                   sampling="4:4:4")
    assert scan.data_ptr() == buf.data_ptr() + 37 and int(length.item()) == n
    host = buf.cpu().numpy()
    assert hip.jpeg_file(header, host[37:37 + n].tobytes()) == want
    assert np.all(host[:37] == 0xA5) and np.all(host[37 + n:] == 0xA5)


@pytest.mark.parametrize("sampling", NEW)
def test_capacity_five_bytes_short(gpu, sampling):
    from vfml import hip
    want = oracle_file("noise150x40", sampling)
    header = hip.jpeg_header(150, 40, 95, sampling)
    n = len(want) - len(header) - 2
    cap = n - 5
    buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    scan, length = hip.jpeg_encode(torch.from_numpy(PICTURES["noise150x40"]).to(gpu), out=buf[:cap], sampling=sampling)
    assert int(length.item()) == n
    with pytest.raises(RuntimeError, match=str(n)):
        hip.jpeg_scan(scan, length)
    host = buf.cpu().numpy()
    assert np.all(host[cap:] == 0xA5)
    assert host[:cap].tobytes() == want[len(header):len(header) + cap]


@pytest.mark.parametrize("name", ["random45x67", "binary33x17", "one1x1", "noise150x40"])
@pytest.mark.parametrize("sampling", NEW)
def test_round_trip_on_the_device(gpu, sampling, name):
    """The device decoder reads the device encoder's file as libjpeg does."""
    from vfml import hip
    data = gpu_file(hip, torch.from_numpy(PICTURES[name]).to(gpu), sampling=sampling)
    info = jp.parse(data, jp.DEVICE_SAMPLINGS)
    assert info.sampling == sampling and jp.decode_plan(info) == "interval"
    rgb, status = hip.jpeg_decode(data, device=gpu)
    assert int(status.item()) == 0
    assert np.array_equal(rgb.cpu().numpy(), pillow_decode(data))


def test_rejected_samplings_launch_nothing(gpu):
    from vfml import hip
    L = hip.lib()
    t = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device=gpu)
    p = ctypes.c_void_p(t.data_ptr())
    for samp in (3, 7, -1):                        # VFML_JPEG_GREY and values outside the enum
        assert L.vfml_jpeg_sampled_workspace_bytes(8, 8, samp) == 0
        assert L.vfml_jpeg_sampled_scan_capacity(8, 8, samp) == 0
        assert L.vfml_jpeg_encode_rgb_sampled(p, 8, 8, 24, samp, p, p, p, 1 << 16, p, None) != 0
        assert b"sampling" in L.vfml_last_error()
    torch.cuda.synchronize()
    assert bool((t == 0xA5).all())                 # picture, tables, workspace, scan and length cell in one: untouched
    with pytest.raises(ValueError, match="4:4:4"):
        hip.jpeg_encode(t[:192].view(8, 8, 3), sampling="grey")
    with pytest.raises(ValueError, match="4:4:4"):
        hip.jpeg_header(8, 8, 95, "grey")
    # the samplings size their own workspaces and scans
    ws = [L.vfml_jpeg_sampled_workspace_bytes(64, 64, s) for s in range(3)]
    cap = [L.vfml_jpeg_sampled_scan_capacity(64, 64, s) for s in range(3)]
    assert 0 < ws[0] < ws[1] < ws[2]
    assert cap == [4 * (4 * 6 * 416 + 2) - 2, 8 * (4 * 4 * 416 + 2) - 2, 8 * (8 * 3 * 416 + 2) - 2]
    assert [hip.jpeg_scan_capacity(64, 64, s) for s in eo.SAMPLINGS] == cap


# ---- flow_processor ---------------------------------------------------------------------------------------------------
def avi_chunks(path):
    from storage.avi_reader import AviReader
    rd, out = AviReader(str(path)), []
    while True:
        at = rd._next_chunk()
        if at is None:
            return out
        rd._f.seek(at[0])
        out.append(rd._f.read(at[1]))


def _run(main, argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = main(argv)
    assert rc == 0, out.getvalue()
    return out.getvalue()


def _only(directory, suffix):
    (path,) = [p for p in directory.iterdir() if p.suffix == suffix]
    return path


FLOW_VIDEO = ["--input", "synthetic:160x128x5", "--sequence-length", "3", "--flow-only", "--flow-format",
              "motion-vectors-rg8", "--device", "cuda"]


@pytest.fixture()
def workdir(tmp_path, monkeypatch):
    from vfml import get_cfg
    from vfml.weights import write_seeded_checkpoint
    write_seeded_checkpoint(str(tmp_path), get_cfg(), seed=0)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("VFML_MJPG_SAMPLING", raising=False)
    return tmp_path


def test_flow_video_at_444_and_its_way_back(gpu, workdir, monkeypatch):
    import flow_processor as fp
    from storage import avi_reader
    monkeypatch.setattr(fp, "MJPG_SAMPLING", "4:4:4")
    first = workdir / "flowvideo"
    first.mkdir()
    log = _run(fp.main, FLOW_VIDEO + ["--output", str(first)])
    assert "MJPG_SAMPLING" not in log
    video = _only(first, ".avi")
    chunks = avi_chunks(video)
    assert len(chunks) == 5
    assert [jp.parse(c, jp.DEVICE_SAMPLINGS).sampling for c in chunks] == ["4:4:4"] * 5
    (cache,) = [p for p in first.iterdir() if p.is_dir()]
    monkeypatch.setattr(avi_reader, "_pillow", lambda: None)      # the device decoder's row-windowed read
    out = workdir / "grid"
    out.mkdir()
    _run(fp.main, ["--input", "synthetic:160x128x5", "--sequence-length", "3", "--taa", "--flow-format",
                   "motion-vectors-rg8", "--device", "cuda", "--use-flow-cache", str(cache), "--flow-input", str(video),
                   "--output", str(out)])
    grid = avi_chunks(_only(out, ".avi"))
    assert len(grid) == 5 and all(jp.parse(c, jp.DEVICE_SAMPLINGS).sampling == "4:4:4" for c in grid)


def test_flow_video_stays_420_by_default(gpu, workdir):
    import flow_processor as fp
    assert fp.MJPG_SAMPLING == "4:2:0"
    first = workdir / "flowvideo"
    first.mkdir()
    log = _run(fp.main, FLOW_VIDEO + ["--output", str(first)])
    (note,) = [line for line in log.splitlines() if "MJPG_SAMPLING" in line]
    assert "4:2:0" in note and "motion edges" in note
    chunks = avi_chunks(_only(first, ".avi"))
    assert [jp.parse(c, jp.DEVICE_SAMPLINGS).sampling for c in chunks] == ["4:2:0"] * 5
