"""The device JPEG decoder's other samplings without a GPU ("Samplings"): the numpy definition
(tests/jpeg_sampling_oracle.py) for 4:4:4, 4:2:2 and grey files against Pillow's decode byte for byte - no tolerance -
the header parser's new argument, row windows, damaged scans, and the C++ steps of the self-synchronising kernels
(vfml/csrc/jpeg_sync_steps.h) run for each sampling by tools/jpeg_sync_host.cpp under ASan + UBSan.  Pillow writes every
fixture; tests/test_gpu_jpeg_sampling.py feeds the same files to the kernels."""
import functools
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_sampling_oracle as so
from jpeg_decode_oracle import JpegError
from storage import jpeg_parse as jp
from storage import jpeg_tables as jt
from test_jpeg_selfsync_cpu import ROOT, _compilers, _results

Image = pytest.importorskip("PIL.Image")

SAMPLINGS = ("4:4:4", "4:2:2", "grey")
# h x w: a single partial MCU, exactly one MCU (of 4:4:4 and grey), odd sizes on both axes, both sides of the rule for
# narrow chroma planes (w <= 4), a last MCU column of one pixel
SIZES = ((1, 1), (8, 8), (9, 17), (17, 33), (7, 3), (7, 4), (7, 5), (40, 6), (45, 67), (3, 130))
RESTARTS = {"norst": {}, "rows1": dict(restart_marker_rows=1), "blocks3": dict(restart_marker_blocks=3)}
QUALITIES = (95, 30)
KINDS = ("random", "smooth")
SAMPLING_CODE = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2, "grey": 3}


@functools.lru_cache(maxsize=None)
def picture(kind, h, w):
    if kind == "random":
        return np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(5 * xx + 2 * yy) % 256, (3 * yy + 40) % 256, (255 - 2 * xx - yy) % 256], axis=-1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pillow_file(sampling, kind, h, w, restart="norst", quality=95):
    """The picture as Pillow writes it: mode L for grey, subsampling= for the others."""
    img = Image.fromarray(picture(kind, h, w), "RGB")
    buf = io.BytesIO()
    if sampling == "grey":
        img.convert("L").save(buf, format="JPEG", quality=quality, **RESTARTS[restart])
    else:
        img.save(buf, format="JPEG", quality=quality, subsampling=sampling, **RESTARTS[restart])
    return buf.getvalue()


def pillow_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def files_of(sampling, h, w):
    """name -> file: the size in every restart setting, quality and kind of picture."""
    return {f"{kind}_{restart}_q{q}": pillow_file(sampling, kind, h, w, restart, q)
            for kind in KINDS for restart in RESTARTS for q in QUALITIES}


@functools.lru_cache(maxsize=None)
def damaged_files(sampling):
    """name -> a 17x33 file whose scan is damaged: cut in half (no markers), and with its restart markers removed."""
    f = pillow_file(sampling, "random", 17, 33, "norst", 95)
    s, e = jp.parse(f, jp.DEVICE_SAMPLINGS).scan
    out = {"half": f[:s + (e - s) // 2] + jt.EOI}
    f = pillow_file(sampling, "random", 17, 33, "rows1", 95)
    s, e = jp.parse(f, jp.DEVICE_SAMPLINGS).scan
    scan = bytearray()
    i = s
    while i < e:
        if f[i] == 0xFF and i + 1 < e and 0xD0 <= f[i + 1] <= 0xD7:
            i += 2
            continue
        scan.append(f[i])
        i += 1
    assert len(scan) < e - s
    out["rst_removed"] = f[:s] + bytes(scan) + f[e:]
    return out


# ---- the oracle against Pillow ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_oracle_equals_pillow(sampling, size):
    for name, data in files_of(sampling, *size).items():
        info = jp.parse(data, jp.DEVICE_SAMPLINGS)
        assert info.sampling == sampling and (info.h, info.w) == size, name
        got, want = so.decode(data), pillow_decode(data)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()))


def test_oracle_restates_the_420_definition():
    """For 4:2:0 the new oracle is the old one: same coefficients path, same filter (wider than 4 pixels it is Pillow's)."""
    import jpeg_decode_oracle as jd
    img = Image.fromarray(picture("random", 45, 67), "RGB")
    for kw in RESTARTS.values():
        buf = io.BytesIO()
        img.save(buf, format="JPEG", quality=90, subsampling="4:2:0", **kw)
        data = buf.getvalue()
        assert np.array_equal(so.decode(data), jd.decode(data))
        assert np.array_equal(so.decode(data), pillow_decode(data))
        assert np.array_equal(so.decode(data, rows=(22, 45)), jd.decode(data, rows=(22, 45)))


def test_restart_marker_numbers_wrap():
    """More than 8 intervals: the marker number goes past RST7."""
    data = pillow_file("4:4:4", "random", 40, 150, "blocks3", 95)
    info = jp.parse(data, jp.DEVICE_SAMPLINGS)
    assert info.mcu_grid == (5, 19) and info.restart_interval == 3 and info.intervals == 32
    cnt = {}
    got = so.decode(data, counters=cnt)
    assert cnt["intervals"] == 32 and cnt["rst_wraps"] >= 3
    assert np.array_equal(got, pillow_decode(data))


# ---- the parser ------------------------------------------------------------------------------------------------------
def test_one_argument_parse_keeps_its_messages():
    with pytest.raises(jp.JpegUnsupported, match=r"sampling factors 2x1 / 1x1 / 1x1; 2x2 / 1x1 / 1x1 \(4:2:0\) only"):
        jp.parse(pillow_file("4:2:2", "random", 17, 33))
    with pytest.raises(jp.JpegUnsupported, match=r"sampling factors 1x1 / 1x1 / 1x1; 2x2 / 1x1 / 1x1 \(4:2:0\) only"):
        jp.parse(pillow_file("4:4:4", "random", 17, 33))
    with pytest.raises(jp.JpegUnsupported, match=r"1 component\(s\); three \(Y Cb Cr\) only"):
        jp.parse(pillow_file("grey", "random", 17, 33))


@pytest.mark.parametrize("sampling, grid", (("4:2:2", (3, 3)), ("4:4:4", (3, 5)), ("grey", (3, 5))))
def test_parse_with_device_samplings(sampling, grid):
    """17x33: MCUs of 8x16, 8x8 and 8x8; the interval count and the kernel the rule picks follow the grid."""
    assert jp.DEVICE_SAMPLINGS == ("4:2:0", "4:2:2", "4:4:4", "grey")
    rows, cols = grid
    for restart, ri, nint, plan in (("norst", 0, 1, "sync"), ("rows1", cols, rows, "interval"),
                                    ("blocks3", 3, -(-rows * cols // 3), "interval" if cols >= 3 else "sync")):
        info = jp.parse(pillow_file(sampling, "random", 17, 33, restart), jp.DEVICE_SAMPLINGS)
        assert info.sampling == sampling and (info.h, info.w) == (17, 33)
        assert info.mcu_grid == grid == jt.mcu_grid(17, 33, sampling)
        assert (info.restart_interval, info.intervals) == (ri, nint), restart
        assert jp.decode_plan(info) == plan, restart
        qt, tables = jp.decode_tables(info)
        assert qt.shape == (3, 64) and qt.dtype == np.uint8 and tables.shape == (jp.TABLE_INTS,)
        if sampling == "grey":
            assert len(info.selectors) == 1
            assert np.array_equal(qt[1], qt[0]) and np.array_equal(qt[2], qt[0])
            assert tuple(tables[2:6]) == (tables[0], tables[1], tables[0], tables[1])
    assert jt.mcu_grid(17, 33) == (2, 3)                 # two-argument calls are 4:2:0's
    info = jp.parse(pillow_file(sampling, "random", 3, 130, "blocks3"), jp.DEVICE_SAMPLINGS)
    assert jp.decode_plan(info) == "interval"            # Ri = 3 is below a row of 9 or 17 MCUs


def _patch_factors(data, factors):
    """The file with its SOF0 sampling factors replaced."""
    at = data.index(b"\xff\xc0")
    out = bytearray(data)
    assert out[at + 9] == 3
    for c, f in enumerate(factors):
        out[at + 11 + 3 * c] = f
    return bytes(out)


def test_what_stays_refused():
    base = pillow_file("4:2:2", "random", 17, 33)
    try:
        buf = io.BytesIO()
        Image.fromarray(picture("random", 17, 33), "RGB").save(buf, format="JPEG", subsampling="4:4:0")
        f440 = buf.getvalue()
    except (TypeError, ValueError, KeyError):            # a Pillow that does not write 4:4:0
        f440 = _patch_factors(base, (0x12, 0x11, 0x11))
    for data, word in ((f440, r"1x2 / 1x1 / 1x1"), (_patch_factors(base, (0x41, 0x11, 0x11)), r"4x1 / 1x1 / 1x1"),
                       (_patch_factors(base, (0x22, 0x11, 0x21)), r"2x2 / 1x1 / 2x1: chroma components whose factors differ")):
        with pytest.raises(jp.JpegUnsupported, match=word) as e:
            jp.parse(data, jp.DEVICE_SAMPLINGS)
        assert "(4:2:0), 2x1 / 1x1 / 1x1 (4:2:2), 1x1 / 1x1 / 1x1 (4:4:4) only" in str(e.value)
    at = base.index(b"\xff\xc0")
    for nf in (2, 4):
        data = bytearray(base)
        data[at + 9] = nf
        with pytest.raises(jp.JpegUnsupported, match=rf"{nf} component\(s\); three \(Y Cb Cr\) or one \(grey\) only"):
            jp.parse(bytes(data), jp.DEVICE_SAMPLINGS)
    # three components in several scans: the first SOS names one of them
    sos = base.index(b"\xff\xda")
    one = base[:sos] + b"\xff\xda" + struct.pack(">H", 8) + bytes([1, 1, 0x00, 0, 63, 0]) + base[sos + 14:]
    with pytest.raises(jp.JpegUnsupported, match="a scan of 1 component.*several scans"):
        jp.parse(one, jp.DEVICE_SAMPLINGS)


# ---- row windows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_row_windows(sampling):
    """45x67: a window is the slice of the whole picture; with one MCU row per interval only the intervals of its luma
    rows are decoded - these samplings have no vertical filter, so no neighbour rows."""
    h = 45
    for restart in RESTARTS:
        data = pillow_file(sampling, "random", h, 67, restart, 95)
        full = so.decode(data)
        for y0, y1 in ((h // 2, h), (0, 1), (7, 9), (8, 16), (44, 45)):
            cnt = {}
            assert np.array_equal(so.decode(data, rows=(y0, y1), counters=cnt), full[y0:y1]), (restart, y0, y1)
            if restart == "rows1":
                assert cnt["intervals"] == 6 and cnt["intervals_decoded"] == (y1 - 1) // 8 - y0 // 8 + 1, (y0, y1)
            else:
                assert cnt["intervals_decoded"] == cnt["intervals"]
    with pytest.raises(ValueError):
        so.decode(data, rows=(3, 3))


# ---- damaged scans ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_damaged_scans_raise(sampling):
    d = damaged_files(sampling)
    with pytest.raises(JpegError, match="ran out|no Huffman table|past"):
        so.decode(d["half"])
    with pytest.raises(JpegError, match="intervals"):
        so.decode(d["rst_removed"])


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cmds = _compilers()
    if not cmds:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("jpeg_sync_host") / "jpeg_sync_host")
    errors = []
    for cmd in cmds:
        done = subprocess.run([*cmd, os.path.join(ROOT, "tools", "jpeg_sync_host.cpp"), "-o", exe], capture_output=True,
                              text=True)
        if done.returncode == 0:
            return exe
        errors.append(done.stderr[-2000:])
    raise AssertionError("\n".join(errors))


def write_case(path, data, S):
    """A case file of tools/jpeg_sync_host.cpp: the sampling rides in the high half of the subsequence-size word."""
    info = jp.parse(data, jp.DEVICE_SAMPLINGS)
    _, tables = jp.decode_tables(info)
    scan = bytes(data[info.scan[0]:info.scan[1]])
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", info.h, info.w, info.restart_interval, S | SAMPLING_CODE[info.sampling] << 16, len(scan)))
        f.write(tables.astype("<i4").tobytes())
        f.write(scan)


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_the_host_program_under_asan_and_ubsan(sampling, host_program, tmp_path):
    """The steps the sync kernels are made of, for this sampling, on the CPU under sanitizers, as a stand-alone child
    process: every size without markers and with 3 MCUs per interval at subsequences of 16 and 128 bytes gives status 0
    and the oracle's coefficients; the damaged files end clean with a non-zero status."""
    cases = [(f"{h}x{w}_{restart}", pillow_file(sampling, "random", h, w, restart, 95), S, True)
             for h, w in SIZES + ((40, 150),) for restart in ("norst", "blocks3") for S in (16, 128)]
    cases += [(name, data, S, False) for name, data in damaged_files(sampling).items() for S in (16, 128)]
    paths = []
    for k, (_, data, S, _) in enumerate(cases):
        paths.append(str(tmp_path / f"case{k}.bin"))
        write_case(paths[-1], data, S)
    done = subprocess.run([host_program, *paths], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    assert "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, done.stderr[-4000:]
    results = _results(done.stdout)
    assert len(results) == len(cases)
    for (name, data, S, whole), (status, subs, coef) in zip(cases, results):
        if not whole:
            assert status != 0, (name, S)
            continue
        assert status == 0, (name, S, status)
        _, want = so.coefficients(data)
        assert np.array_equal(coef, want.reshape(-1, 64).astype(np.int16)), (name, S)
