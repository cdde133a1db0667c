"""The self-synchronising JPEG entropy decoder without a GPU: its Python definition
(tests/jpeg_selfsync_oracle.py) against the serial oracle's coefficients on every file, the hard paths those files reach
(speculation that agrees late or never, blocks across several subsequences, stuffing cut by an edge, markers inside a
subsequence, poisoned speculation), the damaged streams, the rule that picks the kernel, and the C++ steps the kernels
are made of (vfml/csrc/jpeg_sync_steps.h) run in series by tools/jpeg_sync_host.cpp under ASan + UBSan."""
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_decode_oracle as jd
import jpeg_oracle as jo
import jpeg_selfsync_oracle as js
from storage import jpeg_parse as jp
from storage import jpeg_tables as jt
from test_jpeg_decode_cpu import PICTURES, damaged_files, own_file, pillow_file, pillow_variant, restart_markers, scan_range

SIZES = (16, 32, 128)
NORST_QUALITIES = (75, 95, 100)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def norst_file(name, quality):
    """Pillow's file of a picture as Pillow writes it by default: no DRI segment, the scan one interval."""
    return pillow_file(PICTURES[name], quality=quality)


@functools.lru_cache(maxsize=None)
def wide_file():
    """24 x 1300 noise of this project's encoder: Ri = 82, intervals of 8 KiB and more (test_gpu_jpeg_decode's)."""
    return jo.encode(np.random.default_rng(17).integers(0, 256, (24, 1300, 3), dtype=np.uint8), 95)


class _Files:
    """name -> file bytes, made when first asked for (a Pillow-written file needs Pillow only where it is used)."""

    def __init__(self):
        self._make = {f"norst_{name}_q{q}": functools.partial(norst_file, name, q)
                      for name in PICTURES for q in NORST_QUALITIES}
        self._make.update({f"pillow_{name}_{v}": functools.partial(pillow_variant, name, v)
                           for name in ("random45x67", "noise150x40") for v in ("rows1_q60", "blocks3_opt_q85")})
        self._make["wide_ri82"] = wide_file
        self._make.update({f"own_{name}_q95": functools.partial(own_file, name, 95) for name in PICTURES})
        self._make["own_noise150x40_q100"] = functools.partial(own_file, "noise150x40", 100)

    def __iter__(self):
        return iter(self._make)

    def __getitem__(self, name):
        return self._make[name]()


FILES = _Files()


def sync_files():
    """name -> file bytes: every file of the self-synchronising decoder's tests."""
    return FILES


@functools.lru_cache(maxsize=None)
def serial(name):
    c = js.serial_coefficients(FILES[name])
    assert np.abs(c).max() < 32768
    return c.astype(np.int16)


@functools.lru_cache(maxsize=None)
def selfsync(name, S):
    return js.decode(FILES[name], S)


RI3_LONG = ("pillow_noise150x40_blocks3_opt_q85", 1024)     # Ri = 3: intervals of some 500 bytes, several per subsequence
CASES = [(name, S) for name in FILES for S in SIZES] + [RI3_LONG, ("pillow_random45x67_blocks3_opt_q85", 1024)]


@pytest.mark.parametrize("name,S", CASES)
def test_coefficients_equal_the_serial_decode(name, S):
    if "norst" in name or "pillow" in name:
        pytest.importorskip("PIL.Image")
    coef, cnt = selfsync(name, S)
    want = serial(name)
    assert cnt["status"] == 0
    assert coef.shape == want.shape and coef.dtype == np.int16
    assert np.array_equal(coef, want), f"{(coef != want).any(axis=-1).sum()} blocks differ"
    scan = scan_range(FILES[name])
    assert cnt["subsequences"] == max(1, -(-(scan[1] - scan[0]) // S))


def test_the_files_reach_the_hard_paths():
    pytest.importorskip("PIL.Image")
    noise = selfsync("norst_noise150x40_q100", 16)[1]
    print("noise q100 S=16:", noise)
    assert noise["late_sync"] > 0 and noise["rounds_max"] >= 3 and noise["straddling_blocks_max"] >= 3
    for S in SIZES:                                  # the later the agreement, the more rounds: both shrink with S
        assert selfsync("norst_noise150x40_q100", S)[1]["rounds_max"] >= 2
    checker = selfsync("norst_checker150x40_q95", 16)[1]
    print("checker q95 S=16:", checker)
    assert checker["never_sync"] > 0
    assert selfsync("norst_frequency150x40_q95", 16)[1]["never_sync"] > 0
    flat = selfsync("norst_flat150x40_q95", 16)[1]
    assert flat["late_sync"] == 0 and flat["never_sync"] <= 1          # agrees in the next subsequence
    split = {(name, S): selfsync(name, S)[1]["split_stuffing"] for name in FILES for S in SIZES}
    assert sum(split.values()) > 0
    assert split[("norst_noise150x40_q100", 16)] > 0
    name, S = RI3_LONG
    ri3 = selfsync(name, S)[1]
    m = restart_markers(FILES[name])
    assert jp.parse(FILES[name]).restart_interval == 3 and ri3["markers_inside"] > 0
    assert selfsync(name, 16)[1]["markers_inside"] == len(m)
    assert min(b - a - 2 for a, b in zip(m, m[1:])) < S                 # an interval shorter than a subsequence
    assert ri3["markers_inside"] < len(m)                               # ... so that one subsequence holds several markers
    assert sum(selfsync(name, S)[1]["poisoned"] for name in FILES for S in SIZES) > 0
    assert noise["poisoned"] > 0


# ---- damaged streams -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def damaged_norst_files():
    """The damaged streams of test_jpeg_decode_cpu rebuilt from files without restart markers where that can be done
    (a removed marker needs markers): a scan cut in half, a stretch of the scan replaced by 00 bytes."""
    out = {}
    f = norst_file("noise150x40", 95)
    s, e = scan_range(f)
    out["norst_half_150x40"] = f[:s + (e - s) // 2] + jt.EOI
    f = norst_file("flat150x40", 95)
    s, e = scan_range(f)
    a, b = s + (e - s) // 3, s + 2 * (e - s) // 3
    out["norst_zeros_150x40"] = f[:a] + bytes(b - a) + f[b:]
    return out


@functools.lru_cache(maxsize=None)
def damaged_flip_files():
    """One bit of a scan of this project's encoder changed, at places where the serial oracle then meets a code that
    is in no Huffman table and a coefficient index past 63: the two errors that the other damaged streams, which all
    end in the marker count or in a scan that runs out, do not reach."""
    f = own_file("random45x67", 95)
    s = scan_range(f)[0]
    flip = lambda at, bit: f[:s + at] + bytes([f[s + at] ^ (1 << bit)]) + f[s + at + 1:]
    return {"flip_code_45x67": flip(3671, 5), "flip_index_45x67": flip(1829, 4)}


DAMAGED_NORST = ["norst_half_150x40", "norst_zeros_150x40"]             # made from Pillow's files
DAMAGED = ["half_32x32", "rst_removed_150x40", "zeros_150x40", "flip_code_45x67", "flip_index_45x67"] + DAMAGED_NORST
FLIP_BITS = {"flip_code_45x67": 4, "flip_index_45x67": 8}


@functools.lru_cache(maxsize=None)
def damaged(name):
    """A damaged file by name; one made from a Pillow-written file skips the test that asks for it without Pillow."""
    if name in DAMAGED_NORST:
        pytest.importorskip("PIL.Image")
        return damaged_norst_files()[name]
    return {**damaged_files(), **damaged_flip_files()}[name]


def have_pillow():
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return False
    return True


def serial_error_bit(data):
    """The VFML_JPEG_ERR_* bit of the error the serial oracle raises."""
    with pytest.raises(jd.JpegError) as e:
        jd.decode(data)
    text = str(e.value)
    for word, bit in (("restart intervals in the scan", 1), ("out of sequence", 2), ("in no Huffman table", 4),
                      ("past coefficient 63", 8), ("index past 63", 8), ("ran out", 16)):
        if word in text:
            return bit
    raise AssertionError(text)


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name", DAMAGED)
def test_damaged_streams_end_in_the_status(name, S):
    data = damaged(name)
    bit = serial_error_bit(data)
    assert bit == FLIP_BITS.get(name, bit)
    _, cnt = js.decode(data, S)
    assert cnt["status"] != 0 and cnt["status"] & bit, (cnt["status"], bit)


def test_status_is_zero_exactly_when_the_serial_decode_succeeds():
    """Single damaged bytes at seeded places of one file: both decoders agree on whether the stream is damaged."""
    data = own_file("random45x67", 95)
    s, e = scan_range(data)
    rng = np.random.default_rng(3)
    seen = set()
    for at in rng.integers(s, e, 40).tolist():
        bad = data[:at] + bytes([data[at] ^ (1 << int(rng.integers(0, 8)))]) + data[at + 1:]
        try:
            jd.decode(bad)
            raised = False
        except jd.JpegError:
            raised = True
        except jp.JpegUnsupported:
            continue
        _, cnt = js.decode(bad, 16)
        assert (cnt["status"] != 0) == raised, at
        seen.add(raised)
    assert seen == {True, False}


# ---- the rule ------------------------------------------------------------------------------------------------------
def test_the_plan_rule():
    from vfml import hip
    info = jp.parse(own_file("random45x67", 95))                       # 3 x 5 MCUs, Ri = 5
    cols = info.mcu_grid[1]
    assert cols == 5 and info.restart_interval == cols
    want = {0: "sync", cols: "interval", cols + 1: "sync", 3: "interval"}
    for ri, plan in want.items():
        info.restart_interval = ri
        assert hip.jpeg_decode_plan(info) == plan == jp.decode_plan(info), ri


def test_the_default_subsequence_size_grows_with_the_scan():
    """128 bytes up to 65536 subsequences (8 MiB), then doubled while it can be: the chain kernel's groups stay few."""
    from vfml import hip
    assert hip.JPEG_SUBSEQ_BYTES == 128
    want = {0: 128, 600_000: 128, 1 << 23: 128, (1 << 23) + 1: 256, 1 << 24: 256, 1 << 26: 1024, (1 << 31) - 1: 1024}
    for n, sub in want.items():
        assert hip.jpeg_subseq_bytes(n) == sub, n


# ---- the C++ steps under sanitizers ----------------------------------------------------------------------------------
def _compilers():
    """Commands that compile the host program with ASan + UBSan, the sanitizer runtime linked statically where the
    compiler can, so that the program needs nothing from its environment."""
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-I",
             os.path.join(ROOT, "video-flow-ml_amd", "vfml", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    out = []
    for cxx in ("c++", "g++", "clang++"):
        if shutil.which(cxx):
            out += [[cxx, *san, "-static-libasan", "-static-libubsan", *flags], [cxx, *san, "-static-libsan", *flags],
                    [cxx, *san, *flags]]
    if shutil.which("hipcc"):
        out.append(["hipcc", "-x", "c++", *(f for s in san for f in ("-Xarch_host", s)), *flags])
    return out


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


def _case(path, data, S):
    info = jp.parse(data)
    _, tables = jp.decode_tables(info)
    scan = bytes(data[info.scan[0]:info.scan[1]])
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", info.h, info.w, info.restart_interval, S, len(scan)))
        f.write(tables.astype("<i4").tobytes())
        f.write(scan)


def _results(text):
    """The program's output -> [(status, subsequences, coef [blocks, 64])]"""
    out = []
    for part in text.split("case ")[1:]:
        lines = part.splitlines()
        status, subs = int(lines[1].split()[1]), int(lines[2].split()[1])
        coef = np.array([[int(v) for v in ln.split()] for ln in lines[3:]], np.int16).reshape(-1, 64)
        out.append((status, subs, coef))
    return out


def test_the_host_program_under_asan_and_ubsan(host_program, tmp_path):
    """Every file and every damaged stream: status and coefficients equal the Python definition's - on a damaged stream
    too, where that pins what is written up to the error and that nothing behind it in that interval is.  Without
    Pillow the files that Pillow writes are left out, not the run."""
    pillow = have_pillow()
    cases = [(name, FILES[name], S) for name, S in CASES if pillow or name.startswith(("own_", "wide_"))]
    cases += [(name, damaged(name), S) for name in DAMAGED if pillow or name not in DAMAGED_NORST for S in SIZES]
    paths = []
    for k, (_, data, S) in enumerate(cases):
        paths.append(str(tmp_path / f"case{k}.bin"))
        _case(paths[-1], data, S)
    done = subprocess.run([host_program, *paths], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    assert "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, done.stderr[-4000:]
    results = _results(done.stdout)
    assert len(results) == len(cases)
    for (name, data, S), (status, subs, coef) in zip(cases, results):
        want, cnt = js.decode(data, S) if name in DAMAGED else selfsync(name, S)
        if name in DAMAGED:
            assert status != 0 and status & serial_error_bit(data), (name, S, status)
        else:
            assert status == 0, (name, S, status)
        assert status == cnt["status"] and subs == cnt["subsequences"], (name, S, status, cnt["status"])
        assert np.array_equal(coef, want.reshape(-1, 64)), (name, S)
