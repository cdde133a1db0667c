"""The project's baseline JPEG without a GPU: storage/jpeg_tables.py against the segments of a
file Pillow writes, the numpy restatement (tests/jpeg_oracle.py) decoded by Pillow and held to Pillow's own quality,
the hard paths its pictures reach, the kernel's generated tables, and AviWriter(encoder='external')."""
import functools
import io
import os
import sys

import numpy as np
import pytest

import jpeg_oracle as jo
from storage import jpeg_tables as jt

PICTURES = jo.pictures()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# PSNR of the oracle's stream against Pillow's own quality-95 encoder, measured: 0.0 to 1.0 dB below it; the margin
# covers the plain +2 chroma rounding and the 13-bit DCT against libjpeg's
PSNR_MARGIN_DB = 1.5


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    counters = {}
    return jo.encode(PICTURES[name], 95, counters), counters


def oracle_file(name):
    return oracle_result(name)[0]


def segments(data):
    """[(marker, segment bytes)] from behind SOI up to and including SOS."""
    assert data[:2] == jt.SOI
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        n = int.from_bytes(data[i + 2:i + 4], 'big')
        out.append((data[i + 1], bytes(data[i:i + 2 + n])))
        i += 2 + n
        if out[-1][0] == 0xDA:
            return out


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-9))


def test_segments_equal_a_pillow_file():
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(PICTURES["random45x67"], "RGB").save(buf, format="JPEG", quality=95)
    theirs = segments(buf.getvalue())
    assert [m for m, _ in theirs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    ours = segments(jt.jpeg_header(45, 67, 95))
    assert [m for m, _ in ours] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert [s for m, s in ours if m != 0xDD] == [s for _, s in theirs]
    assert dict(ours)[0xDD] == b'\xff\xdd\x00\x04\x00\x05'         # one MCU row of a 67-wide picture: 5 MCUs
    assert [jt.app0_segment(), *jt.dqt_segments(95), jt.sof0_segment(45, 67), *jt.dht_segments(),
            jt.sos_segment()] == [s for _, s in theirs]


def test_quality_scaling_and_dct_matrix():
    q = jt.quant_tables(95)
    assert q.shape == (2, 64) and q[0, 0] == 2 and q[1, 63] == 10
    assert jt.quant_tables(100).max() == 1 and jt.quant_tables(50)[0, 0] == 16 and jt.quant_tables(1).max() == 255
    with pytest.raises(ValueError):
        jt.quant_tables(0)
    c = jt.dct_matrix()
    assert np.all(c[0] == 2896) and np.abs(c).max() == 4017


def test_generated_kernel_tables_are_current():
    sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd", "vfml", "csrc"))
    try:
        import make_jpeg_tables
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "video-flow-ml_amd", "vfml", "csrc", "jpeg_tables.inc")) as f:
        assert f.read() == make_jpeg_tables.render()


@pytest.mark.parametrize("name", list(PICTURES))
def test_pillow_decodes_the_oracle_stream(name):
    Image = pytest.importorskip("PIL.Image")
    img = PICTURES[name]
    dec = np.asarray(Image.open(io.BytesIO(oracle_file(name))).convert("RGB"))
    assert dec.shape == img.shape
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=95)
    ref = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    ours, theirs = psnr(dec, img), psnr(ref, img)
    print(f"{name}: PSNR {ours:.2f} dB, Pillow's encoder {theirs:.2f} dB, {len(oracle_file(name))} bytes "
          f"against {len(buf.getvalue())}")
    assert ours >= theirs - PSNR_MARGIN_DB


def test_the_pictures_reach_the_hard_paths():
    cnt = {name: oracle_result(name)[1] for name in PICTURES}
    for name in ("noise150x40", "checker150x40", "flat150x40", "frequency150x40"):
        assert cnt[name]["rst"] >= 9, name              # ten MCU rows: the marker counter wraps to RST0
    assert cnt["noise150x40"]["stuffed"] > 0 and cnt["checker150x40"]["stuffed"] > 0
    assert cnt["noise150x40"]["max_ac_size"] >= 9
    assert cnt["frequency150x40"]["long_runs"] > 0 and cnt["frequency150x40"]["zrl"] > 0
    assert cnt["flat150x40"]["eob_only"] == 10 * 3 * 6   # every block of the picture
    assert cnt["one1x1"]["rst"] == 0


def test_restart_markers_count_modulo_eight():
    data = oracle_file("flat150x40")
    scan = data[len(jt.jpeg_header(150, 40, 95)):-2]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0]
    assert marks == [0xD0 + (i & 7) for i in range(9)]


def test_avi_writer_external_round_trip(tmp_path, monkeypatch):
    from storage import avi_writer
    from storage.avi_reader import AviReader, probe
    monkeypatch.setattr(avi_writer, "_pillow", lambda: None)            # the writer must not need Pillow
    files = [jo.encode(PICTURES["gradient48x64"], q) for q in (95, 50, 100)]
    path = str(tmp_path / "external.avi")
    wr = avi_writer.AviWriter(path, 'MJPG', 25.0, (64, 48), encoder='external')
    assert wr.mjpg and wr.in_flight_limit() == 0 and wr.in_flight() == 0
    for data in files:
        wr.write_encoded(data)
    with pytest.raises(ValueError):
        wr.write_payload(PICTURES["gradient48x64"])
    wr.drain()
    wr.release()
    assert probe(path) == {"frames": 3, "fps": 25.0, "width": 64, "height": 48, "codec": "MJPG"}
    rd = AviReader(path)
    chunks = []
    while True:
        at = rd._next_chunk()
        if at is None:
            break
        rd._f.seek(at[0])
        chunks.append(rd._f.read(at[1]))
    assert chunks == files
    pytest.importorskip("PIL")
    frames = list(AviReader(path))
    assert len(frames) == 3 and psnr(frames[0], PICTURES["gradient48x64"]) > 35
    plain = avi_writer.AviWriter(str(tmp_path / "plain.avi"), 0, 25.0, (64, 48))
    with pytest.raises(ValueError):
        plain.write_encoded(files[0])
    plain.release()
