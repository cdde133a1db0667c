"""The encoder's samplings without a GPU ("Samplings"): the numpy definition
(tests/jpeg_encode_sampling_oracle.py) at 4:2:2 and 4:4:4 read by Pillow and by storage/jpeg_parse.py, its segments against
Pillow's files of the same subsampling, its 4:2:0 against tests/jpeg_oracle.py, its quality against Pillow's own encoder,
what the samplings do to a motion edge of an rg8 flow picture, the hard paths at 4:4:4, and the sampling on its way
through jpeg_header, AviWriter and flow_processor."""
import contextlib
import functools
import io

import numpy as np
import pytest

import jpeg_encode_sampling_oracle as eo
import jpeg_oracle as jo
from storage import jpeg_parse as jp
from storage import jpeg_tables as jt
from test_jpeg_cpu import PSNR_MARGIN_DB, psnr, segments

PICTURES = jo.pictures()
NEW = ("4:2:2", "4:4:4")
PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


@functools.lru_cache(maxsize=None)
def oracle_result(name, sampling):
    counters = {}
    return eo.encode(PICTURES[name], 95, sampling, counters), counters


def oracle_file(name, sampling):
    return oracle_result(name, sampling)[0]


def pillow_file(img, sampling, quality=95):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=quality, subsampling=PILLOW_SUBSAMPLING[sampling])
    return buf.getvalue()


def pillow_decode(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", list(PICTURES))
def test_420_is_the_existing_definition(name):
    img = PICTURES[name]
    assert eo.encode_scan(img, 95, "4:2:0") == jo.encode_scan(img, 95)
    assert eo.encode(img, 95, "4:2:0") == jo.encode(img, 95)
    assert eo.encode(img, 50) == jo.encode(img, 50)


@pytest.mark.parametrize("name", list(PICTURES))
@pytest.mark.parametrize("sampling", NEW)
def test_pillow_and_the_parser_read_the_file(sampling, name):
    img, data = PICTURES[name], oracle_file(name, sampling)
    assert pillow_decode(data).shape == img.shape
    info = jp.parse(data, jp.DEVICE_SAMPLINGS)
    assert (info.h, info.w, info.sampling) == (*img.shape[:2], sampling)
    assert info.restart_interval == jt.mcu_grid(*img.shape[:2], sampling)[1]
    assert jp.decode_plan(info) == 'interval'
    theirs = dict(_grouped(segments(pillow_file(img, sampling))))
    ours = dict(_grouped(segments(data)))
    for marker in (0xDB, 0xC4, 0xC0, 0xDA):
        assert ours[marker] == theirs[marker], hex(marker)


def _grouped(segs):
    out = {}
    for marker, seg in segs:
        out.setdefault(marker, []).append(seg)
    return out.items()


@pytest.mark.parametrize("name", list(PICTURES))
@pytest.mark.parametrize("sampling", NEW)
def test_quality_against_pillows_encoder(sampling, name):
    img = PICTURES[name]
    theirs_file = pillow_file(img, sampling)
    ours, theirs = psnr(pillow_decode(oracle_file(name, sampling)), img), psnr(pillow_decode(theirs_file), img)
    print(f"{name} {sampling}: PSNR {ours:.2f} dB, Pillow's encoder {theirs:.2f} dB, {len(oracle_file(name, sampling))} "
          f"bytes against {len(theirs_file)}")
    assert ours >= theirs - PSNR_MARGIN_DB


def test_motion_edge_survives_444():
    """Max error in R and G: 4:4:4 < 4:2:2 < 4:2:0, and fewer than 2 % of the 4:4:4 values off by more than 2 levels
    (measured: 56 / 40 / 5 levels, mean 2.25 / 1.48 / 0.43, above 2 levels 14.4 % / 7.1 % / 1.0 %)."""
    img = eo.motion_edge_picture()
    assert img.shape == (48, 64, 3) and sorted(np.unique(img[..., 0])) == [68, 207] and sorted(np.unique(img[..., 1])) == [80, 163]
    got = {}
    for sampling in eo.SAMPLINGS:
        got[sampling] = eo.motion_edge_error(img, pillow_decode(eo.encode(img, 95, sampling)))
        print(f"{sampling}: max {got[sampling][0]} levels, mean {got[sampling][1]:.2f}, above 2 levels "
              f"{100 * got[sampling][2]:.1f} %")
    assert got["4:4:4"][0] < got["4:2:2"][0] < got["4:2:0"][0]
    assert got["4:4:4"][2] < 0.02


def test_444_reaches_the_hard_paths():
    cnt = {name: oracle_result(name, "4:4:4")[1] for name in PICTURES}
    for name in ("noise150x40", "checker150x40", "flat150x40", "frequency150x40"):
        assert cnt[name]["rst"] == 18, name             # 19 MCU rows of 8: the marker counter wraps twice
    data = oracle_file("flat150x40", "4:4:4")
    scan = data[len(jt.jpeg_header(150, 40, 95, "4:4:4")):-2]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0]
    assert marks == [0xD0 + (i & 7) for i in range(18)]
    assert cnt["noise150x40"]["stuffed"] > 0 and cnt["checker150x40"]["stuffed"] > 0
    assert cnt["frequency150x40"]["zrl"] > 0 and cnt["frequency150x40"]["long_runs"] > 0
    assert cnt["flat150x40"]["eob_only"] == 19 * 5 * 3  # every block of the picture
    assert oracle_result("flat150x40", "4:2:2")[1]["eob_only"] == 19 * 3 * 4
    assert cnt["one1x1"]["rst"] == 0


def test_header_names_the_sampling():
    base = jt.jpeg_header(45, 67, 95)
    assert jt.jpeg_header(45, 67, 95, "4:2:0") == base and jt.sof0_segment(45, 67) == jt.sof0_segment(45, 67, "4:2:0")
    for sampling, luma, dri in (("4:2:0", 0x22, 5), ("4:2:2", 0x21, 5), ("4:4:4", 0x11, 9)):
        segs = dict(segments(jt.jpeg_header(45, 67, 95, sampling)))
        assert segs[0xC0][11] == luma and segs[0xDD] == b'\xff\xdd\x00\x04' + dri.to_bytes(2, 'big')
        other = [s for m, s in segments(jt.jpeg_header(45, 67, 95, sampling)) if m not in (0xC0, 0xDD)]
        assert other == [s for m, s in segments(base) if m not in (0xC0, 0xDD)]
    for bad in ("grey", "4:1:1", None, 2):
        with pytest.raises(ValueError, match="4:2:0, 4:2:2, 4:4:4"):
            jt.jpeg_header(45, 67, 95, bad)
        with pytest.raises(ValueError, match="4:2:0, 4:2:2, 4:4:4"):
            jt.sof0_segment(45, 67, bad)


def avi_chunks(path):
    from storage.avi_reader import AviReader
    rd, out = AviReader(str(path)), []
    while True:
        at = rd._next_chunk()
        if at is None:
            return out
        rd._f.seek(at[0])
        out.append(rd._f.read(at[1]))


@pytest.mark.parametrize("sampling", eo.SAMPLINGS)
def test_avi_writer_pillow_writes_the_sampling(tmp_path, sampling):
    pytest.importorskip("PIL")
    from storage.avi_writer import AviWriter
    img = PICTURES["gradient48x64"]
    wr = AviWriter(str(tmp_path / "a.avi"), 'MJPG', 25.0, (64, 48), encoder='pillow', sampling=sampling, workers=2)
    for k in range(3):
        wr.write(np.roll(img, k, axis=1)[:, :, ::-1])
    wr.release()
    chunks = avi_chunks(tmp_path / "a.avi")
    assert len(chunks) == 3
    assert [jp.parse(c, jp.DEVICE_SAMPLINGS).sampling for c in chunks] == [sampling] * 3
    assert psnr(pillow_decode(chunks[0]), img) > 35
    with pytest.raises(ValueError, match="4:4:4"):
        AviWriter(str(tmp_path / "b.avi"), 'MJPG', 25.0, (64, 48), sampling="grey")


def _write_cache(path, n, h, w):
    from storage import FlowCacheManager
    path.mkdir()
    rng = np.random.default_rng(3)
    for i in range(n):
        FlowCacheManager().save_flow_to_cache(rng.normal(0, 3, (h, w, 2)).astype(np.float32), str(path), i, 'npz')


def _flow_processor(tmp_path, name, extra=()):
    import flow_processor as fp
    out = tmp_path / name
    out.mkdir()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = fp.main(["--input", "synthetic:64x48x4", "--output", str(out), "--device", "cpu", "--use-flow-cache",
                      str(tmp_path / "cache"), *extra])
    assert rc == 0, buf.getvalue()
    (avi,) = [p for p in out.iterdir() if p.suffix == ".avi"]
    return [jp.parse(c, jp.DEVICE_SAMPLINGS).sampling for c in avi_chunks(avi)], buf.getvalue()


def test_flow_processor_setting(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    import flow_processor as fp
    monkeypatch.delenv("VFML_MJPG_SAMPLING", raising=False)
    _write_cache(tmp_path / "cache", 4, 48, 64)
    assert fp.MJPG_SAMPLING == "4:2:0" and fp.mjpg_sampling() == "4:2:0"
    flow_only = ("--flow-only", "--flow-format", "motion-vectors-rg8")
    kinds, log = _flow_processor(tmp_path, "default", flow_only)
    assert kinds == ["4:2:0"] * 4
    (note,) = [line for line in log.splitlines() if "MJPG_SAMPLING" in line]
    assert "4:2:0" in note and "motion edges" in note and "loses its vectors" in note
    kinds, log = _flow_processor(tmp_path, "gamedev")
    assert kinds == ["4:2:0"] * 4 and "MJPG_SAMPLING" not in log
    monkeypatch.setattr(fp, "MJPG_SAMPLING", "4:4:4")
    kinds, log = _flow_processor(tmp_path, "set", flow_only)
    assert kinds == ["4:4:4"] * 4 and "MJPG_SAMPLING" not in log
    monkeypatch.setenv("VFML_MJPG_SAMPLING", "4:2:2")              # the environment overrides the module setting
    kinds, _ = _flow_processor(tmp_path, "env")
    assert kinds == ["4:2:2"] * 4
    for bad in ("grey", "444"):
        monkeypatch.setenv("VFML_MJPG_SAMPLING", bad)
        with pytest.raises(ValueError, match="VFML_MJPG_SAMPLING.*4:2:0, 4:2:2, 4:4:4"):
            _flow_processor(tmp_path, "bad" + bad)
        assert not [p for p in (tmp_path / ("bad" + bad)).iterdir() if p.suffix == ".avi"]
    monkeypatch.delenv("VFML_MJPG_SAMPLING")
    monkeypatch.setattr(fp, "MJPG_SAMPLING", "4:1:1")
    with pytest.raises(ValueError, match="flow_processor.MJPG_SAMPLING"):
        fp.mjpg_sampling()
