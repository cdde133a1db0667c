"""The device JPEG decoder's definition without a GPU: the numpy restatement
(tests/jpeg_decode_oracle.py) against Pillow's decode byte for byte - no tolerance - on the project's own files and on
Pillow-written ones, the hard paths those files reach, row windows, the header parser (storage/jpeg_parse.py) and the
damaged streams that the GPU test feeds to the kernels."""
import functools
import io

import numpy as np
import pytest

import jpeg_decode_oracle as jd
import jpeg_oracle as jo
from storage import jpeg_parse as jp
from storage import jpeg_tables as jt

PICTURES = jo.pictures()
QUALITIES = (10, 95, 100)
PILLOW_VARIANTS = {
    "rows1_q60": dict(quality=60, restart_marker_rows=1),
    "blocks3_opt_q85": dict(quality=85, restart_marker_blocks=3, optimize=True),     # Ri = 3: no multiple of an MCU row
    "norst_q95": dict(quality=95),                                                   # Ri = 0
}
WINDOWS = ((75, 150), (37, 90), (0, 1), (149, 150))


def _image():
    """Pillow, asked for where a test needs it: without it that test skips, the others still run."""
    return pytest.importorskip("PIL.Image")


def pillow_file(img, **kw):
    buf = io.BytesIO()
    _image().fromarray(img, "RGB").save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pillow_decode(data):
    return np.asarray(_image().open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=None)
def own_file(name, quality):
    return jo.encode(PICTURES[name], quality)


@functools.lru_cache(maxsize=None)
def pillow_variant(name, variant):
    return pillow_file(PICTURES[name], **PILLOW_VARIANTS[variant])


class _Files:
    """name -> file bytes, made when first asked for: a Pillow-written file needs Pillow only in the test that uses it."""

    def __init__(self):
        self._make = {f"{name}_q{q}": functools.partial(own_file, name, q) for name in PICTURES for q in QUALITIES}
        self._make.update({f"pillow_{name}_{v}": functools.partial(pillow_variant, name, v)
                           for name in ("random45x67", "noise150x40") for v in PILLOW_VARIANTS})

    def __iter__(self):
        return iter(self._make)

    def __getitem__(self, name):
        return self._make[name]()


_FILES = _Files()


def all_files():
    """name -> file bytes: every file of this test, the project's own and Pillow's."""
    return _FILES


@functools.lru_cache(maxsize=None)
def oracle_decode(name):
    """-> (picture, counters) of all_files()[name], decoded once."""
    counters = {}
    return jd.decode(all_files()[name], counters=counters), counters


def scan_range(data):
    return jp.parse(data).scan


def restart_markers(data):
    """Offsets in the file of the scan's RSTm markers."""
    s, e = scan_range(data)
    return [i for i in range(s, e - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


@functools.lru_cache(maxsize=None)
def damaged_files():
    """name -> a file whose scan is damaged: the oracle raises JpegError on each."""
    smooth = np.kron(PICTURES["smooth16x16"], np.ones((2, 2, 1), np.uint8))          # 32 x 32: two intervals
    f = jo.encode(smooth, 95)
    s, e = scan_range(f)
    out = {"half_32x32": f[:s + (e - s) // 2] + jt.EOI}
    f = own_file("noise150x40", 95)
    m = restart_markers(f)
    out["rst_removed_150x40"] = f[:m[2]] + f[m[2] + 2:]
    f = own_file("flat150x40", 95)
    m = restart_markers(f)
    out["zeros_150x40"] = f[:m[3] + 2] + bytes(m[4] - m[3] - 2) + f[m[4]:]           # interval 4 replaced by 00 bytes
    return out


@pytest.mark.parametrize("name", list(all_files()))
def test_oracle_equals_pillow(name):
    data = all_files()[name]
    got, want = oracle_decode(name)[0], pillow_decode(data)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ"


def test_the_files_reach_the_hard_paths():
    cnt = {name: oracle_decode(name)[1] for name in all_files()}
    for name in ("noise150x40", "checker150x40", "flat150x40", "frequency150x40"):
        assert cnt[f"{name}_q95"]["intervals"] >= 9 and cnt[f"{name}_q95"]["rst_wraps"] >= 1, name
    assert cnt["noise150x40_q95"]["stuffed"] > 0 and cnt["checker150x40_q95"]["stuffed"] > 0
    assert cnt["frequency150x40_q95"]["zrl"] > 0
    assert cnt["flat150x40_q95"]["eob_only"] == 10 * 3 * 6
    assert cnt["noise150x40_q100"]["max_ac_size"] >= 9
    assert cnt["pillow_noise150x40_blocks3_opt_q85"]["own_tables"]
    assert not cnt["noise150x40_q95"]["own_tables"] and not cnt["pillow_noise150x40_norst_q95"]["own_tables"]
    assert cnt["pillow_noise150x40_norst_q95"]["intervals"] == 1
    assert cnt["pillow_noise150x40_blocks3_opt_q85"]["intervals"] == 10            # 30 MCUs, Ri = 3
    assert jp.parse(all_files()["pillow_random45x67_blocks3_opt_q85"]).restart_interval == 3
    assert cnt["one1x1_q95"]["intervals"] == 1


@pytest.mark.parametrize("rows", WINDOWS)
@pytest.mark.parametrize("name", ["noise150x40_q95", "pillow_noise150x40_rows1_q60", "pillow_noise150x40_blocks3_opt_q85",
                                  "pillow_noise150x40_norst_q95"])
def test_row_windows(name, rows):
    counters = {}
    got = jd.decode(all_files()[name], rows=rows, counters=counters)
    assert np.array_equal(got, oracle_decode(name)[0][rows[0]:rows[1]])
    info = jp.parse(all_files()[name])
    windowed = info.restart_interval == 3                    # one MCU row of the 40-wide picture; Pillow's Ri = 0 is not
    assert windowed == (name != "pillow_noise150x40_norst_q95")
    if windowed and rows in ((75, 150), (37, 90)):
        assert counters["intervals_decoded"] < counters["intervals"] == 10
    if windowed:
        want = {(75, 150): 6, (37, 90): 4, (0, 1): 1, (149, 150): 1}[rows]
        assert counters["intervals_decoded"] == want
    else:
        assert counters["intervals_decoded"] == counters["intervals"]


def test_row_window_with_intervals_that_are_no_mcu_rows():
    name = "pillow_random45x67_blocks3_opt_q85"             # Ri = 3 in rows of 5 MCUs: the whole picture is decoded
    counters = {}
    got = jd.decode(all_files()[name], rows=(20, 45), counters=counters)
    assert np.array_equal(got, oracle_decode(name)[0][20:45])
    assert counters["intervals_decoded"] == counters["intervals"] == 5


# ---- the parser ----------------------------------------------------------------------------------------------------
def _at(data, marker):
    """Offset of the first segment with `marker`."""
    i = 2
    while data[i + 1] != marker:
        i += 2 + int.from_bytes(data[i + 2:i + 4], 'big')
    return i


def _patched(data, at, value):
    return data[:at] + bytes([value]) + data[at + 1:]


def test_parser_reads_the_project_header():
    data = own_file("random45x67", 95)
    info = jp.parse(data)
    assert (info.h, info.w, info.restart_interval, info.mcu_grid, info.intervals) == (45, 67, 5, (3, 5), 3)
    q = jt.quant_tables(95)
    assert np.array_equal(info.qtables, q[[0, 1, 1]])
    assert info.huffman == jt.HUFFMAN and info.selectors == ((0, 0), (1, 1), (1, 1)) and not info.annex_k
    assert info.scan == (len(jt.jpeg_header(45, 67, 95)), len(data) - 2)
    # COM and APPn segments are skipped, what follows EOI is ignored
    sof = _at(data, 0xC0)
    extra = data[:sof] + b'\xff\xfe\x00\x05abc' + b'\xff\xe5\x00\x04\xff\xd9' + data[sof:] + b'\0\0padding'
    assert np.array_equal(jd.decode(extra), oracle_decode("random45x67_q95")[0])
    qt, tables = jp.decode_tables(info)
    assert qt.shape == (3, 64) and qt.dtype == np.uint8 and tables.shape == (jp.TABLE_INTS,) and tables.dtype == np.int32
    assert tables[:6].tolist() == [0, 1, 2, 3, 2, 3]
    limit, offset = jp.huffman_lookup(jt.DC_LUMA)
    assert limit[:3] == [0, 1 << 14, 7 << 13] and limit[15] == limit[8] == 0xFF80 and offset[1] == 0


def test_the_scan_ends_at_the_first_eoi():
    """What follows EOI is ignored, a second JPEG file with restart markers and an EOI of its own included."""
    data = own_file("random45x67", 95)
    want = jp.parse(data).scan
    assert want[1] == len(data) - 2
    for tail in (own_file("noise150x40", 95), b'\xff\xd0\xff\xd9', b'\0' * 7):
        assert jp.parse(data + tail).scan == want
        assert np.array_equal(jd.decode(data + tail), oracle_decode("random45x67_q95")[0])
    assert jp.parse(data[:-2]).scan == (want[0], len(data) - 2)           # no EOI: the scan runs to the end


UNSUPPORTED = {
    "SOF1": (lambda d: _patched(d, _at(d, 0xC0) + 1, 0xC1), "SOF1"),
    "SOF2": (lambda d: _patched(d, _at(d, 0xC0) + 1, 0xC2), "progressive"),
    "arithmetic": (lambda d: _patched(d, _at(d, 0xC0) + 1, 0xC9), "arithmetic"),
    "12-bit": (lambda d: _patched(d, _at(d, 0xC0) + 4, 12), "12-bit"),
    "16-bit tables": (lambda d: _patched(d, _at(d, 0xDB) + 4, 0x10), "16-bit"),
    "1 component": (lambda d: _patched(d, _at(d, 0xC0) + 9, 1), "1 component"),
    "4 components": (lambda d: _patched(d, _at(d, 0xC0) + 9, 4), "4 component"),
    "sampling": (lambda d: _patched(d, _at(d, 0xC0) + 11, 0x21), "sampling"),
    "several scans": (lambda d: _patched(d, _at(d, 0xDA) + 4, 1), "several scans"),
    "DNL": (lambda d: _patched(d, _at(d, 0xDD) + 1, 0xDC), "DNL"),
    "DNL by zero lines": (lambda d: _patched(_patched(d, _at(d, 0xC0) + 5, 0), _at(d, 0xC0) + 6, 0), "DNL"),
}


@pytest.mark.parametrize("case", list(UNSUPPORTED))
def test_parser_names_what_it_does_not_take(case):
    patch, word = UNSUPPORTED[case]
    with pytest.raises(jp.JpegUnsupported, match=word):
        jp.parse(patch(own_file("random45x67", 95)))
    with pytest.raises(jp.JpegUnsupported, match=word):
        jd.decode(patch(own_file("random45x67", 95)))


def test_a_file_without_dht_gets_the_annex_k_tables():
    h, w = 45, 67
    header = b''.join([jt.SOI, jt.app0_segment(), *jt.dqt_segments(95), jt.sof0_segment(h, w),
                       jt.dri_segment(jt.mcu_grid(h, w)[1]), jt.sos_segment()])
    data = jt.jpeg_file(header, jo.encode_scan(PICTURES["random45x67"], 95))
    assert jp.parse(data).annex_k and jp.parse(data).huffman == jt.HUFFMAN
    assert np.array_equal(jd.decode(data), oracle_decode("random45x67_q95")[0])


def test_read_chunk_hands_out_the_file_bytes(tmp_path):
    from storage.avi_reader import AviReader
    from storage.avi_writer import AviWriter
    path = str(tmp_path / "small.avi")
    wr = AviWriter(path, 'MJPG', 25.0, (64, 48), encoder='external')
    files = [own_file("gradient48x64", q) for q in (95, 10)]
    wr.write_encoded(files[0])
    wr.write_encoded(b'')                         # a dropped frame: repeat
    wr.write_encoded(files[1])
    wr.release()
    with AviReader(path) as a, AviReader(path) as b:
        chunks = [a.read_chunk() for _ in range(4)]
        frames = [b.read() for _ in range(4)]
    assert chunks == [files[0], b'', files[1], None] and a.pos == 3
    assert frames[3] is None and np.array_equal(frames[1], frames[0])
    for chunk, frame in zip((files[0], files[0], files[1]), frames):
        assert np.array_equal(jd.decode(chunk), frame)


# ---- damaged streams -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["half_32x32", "rst_removed_150x40", "zeros_150x40"])
def test_damaged_streams_raise(name):
    data = damaged_files()[name]
    jp.parse(data)                                # the header is whole
    with pytest.raises(jd.JpegError):
        jd.decode(data)


def test_the_zero_interval_runs_out_of_data():
    with pytest.raises(jd.JpegError, match="ran out"):
        jd.decode(damaged_files()["zeros_150x40"])
    with pytest.raises(jd.JpegError, match="intervals"):
        jd.decode(damaged_files()["rst_removed_150x40"])


@pytest.mark.parametrize("name", ["random45x67_q95", "pillow_noise150x40_blocks3_opt_q85"])
def test_lookup_tables_decode_every_code(name):
    """decode_tables' limit / offset form (what the kernel reads) against the canonical codes, for every code of the
    file's four tables with the bits behind it all 0 and all 1."""
    info = jp.parse(all_files()[name])
    _, tables = jp.decode_tables(info)
    for k, table in enumerate(info.huffman):
        base = 8 + 96 * k
        limit, offset = tables[base:base + 16].tolist(), tables[base + 16:base + 32].tolist()
        vals = tables[base + 32:base + 96].view(np.uint8)
        assert np.all(np.diff(limit) >= 0) and limit[15] <= 1 << 16
        for sym, (code, length) in jt.huffman_codes(table).items():
            for tail in (0, (1 << (16 - length)) - 1):
                v = code << (16 - length) | tail
                got = next(l for l in range(1, 17) if v < limit[l - 1])
                assert got == length and vals[offset[length - 1] + (v >> (16 - length))] == sym
