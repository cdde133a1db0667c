"""The flow cache's deflate stream without a GPU: the numpy oracle (tests/deflate_oracle.py)
against zlib, its own inflater and np.load of an assembled archive; the chunk index in the zip extra field; the size
condition against the host writer; and the code-construction header (vfml/csrc/deflate_code.h) run by
tools/deflate_code_host.cpp under ASan + UBSan against the oracle's lengths and codes."""
import os
import shutil
import struct
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

import deflate_oracle as do
from storage import cache_manager as cm
from storage import device_npz as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD = do.flow_field(96, 128, seed=3)


def _rng_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def arrays():
    """name -> (float32 array, chunk_bytes): every kind of chunk, edge lengths in whole floats."""
    C = 1024
    f = FIELD.reshape(-1)
    out = {
        "one_float": (f[:1].copy(), C), "C-4": (f[:C // 4 - 1].copy(), C), "C": (f[:C // 4].copy(), C),
        "C+4": (f[:C // 4 + 1].copy(), C), "3C+20": (f[:3 * C // 4 + 5].copy(), C),
        "field_1024": (FIELD, 1024), "field_4096": (FIELD, 4096), "field_32768": (FIELD, 32768),
        "constant": (np.full(700, 1.5, np.float32), C),
        "random_bits": (np.frombuffer(_rng_bytes(4, 3 * C + 4), np.float32).copy(), C),
        "fibonacci": (np.frombuffer(do.fibonacci_chunk(), np.float32).copy(), 4096),
        "deep": (np.frombuffer(do.deep_chunk(), np.float32).copy(), 8192),
    }
    return out


ARRAYS = arrays()


def oracle_member(name, arr, C):
    """The ZipMember storage/device_npz.py assembles, its stream coded by the oracle in the device's place."""
    stream, offsets, crc, kinds = do.deflate(arr.tobytes(), C, dn.head_crc(arr.shape))
    return dn.assemble_member(name, arr.shape, stream, crc, offsets, C), kinds


@pytest.mark.parametrize("name", list(ARRAYS))
def test_three_decoders_return_the_input(name, tmp_path):
    arr, C = ARRAYS[name]
    raw = arr.tobytes()
    stream, offsets, crc, kinds = do.deflate(raw, C, 0x1234)
    assert zlib.decompress(stream, -15) == raw
    assert do.inflate(stream, offsets, C, len(raw)) == (raw, 0)
    assert crc == zlib.crc32(raw, 0x1234) and do.crc32_table(raw, 0x1234) == crc
    member, _ = oracle_member('flow', arr, C)
    path = str(tmp_path / "a.npz")
    cm.write_npz(path, {'flow': member, 'frame_idx': 7, 'shape': arr.shape, 'dtype': 'float32'}, mode='huffman')
    with np.load(path) as z:
        assert list(z.files) == ['flow', 'frame_idx', 'shape', 'dtype']
        got = z['flow']
        assert got.dtype == np.float32 and got.shape == arr.shape and got.tobytes() == raw
        assert int(z['frame_idx']) == 7 and tuple(z['shape']) == arr.shape and str(z['dtype']) == 'float32'
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        info = z.getinfo('flow.npy')
        assert info.compress_type == zipfile.ZIP_DEFLATED and info.CRC == zlib.crc32(raw, dn.head_crc(arr.shape))


def test_the_kinds_of_chunk_are_all_there():
    assert set(oracle_member('flow', *ARRAYS["random_bits"])[1]) == {"stored"}
    assert set(oracle_member('flow', *ARRAYS["field_4096"])[1]) == {"dynamic"}
    count = np.bincount(np.frombuffer(do.deep_chunk(), np.uint8), minlength=257)
    count[256] = 1
    assert max(do.code_lengths(count.tolist(), 40)) > 15 and max(do.code_lengths(count.tolist(), 15)) == 15
    for limit in (7, 15):          # a complete code whatever the limit does
        for hist in histograms():
            if hist[0] == limit:
                lens = do.code_lengths(hist[1], limit)
                assert max(lens) <= limit
                used = [ln for ln in lens if ln]
                assert len(used) == sum(1 for c in hist[1] if c)
                assert len(used) == 1 or sum(2 ** (limit - ln) for ln in used) == 2 ** limit


def test_host_writer_files_are_unchanged_by_the_refactoring(tmp_path):
    """write_npz lays out what it did before it was split into host_member + write_zip: no extra field, same bytes as a
    layout made here by hand."""
    path = str(tmp_path / "h.npz")
    cm.write_npz(path, {'flow': FIELD, 'frame_idx': 3}, mode='huffman')
    data = open(path, 'rb').read()
    assert struct.unpack_from('<H', data, 28)[0] == 0                      # local header: extra length 0
    with zipfile.ZipFile(path) as z:
        assert all(i.extra == b'' for i in z.infolist()) and z.testzip() is None
    co = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    head = dn.npy_head(FIELD.shape)
    want = co.compress(head) + co.compress(FIELD.tobytes()) + co.flush()
    assert data[30 + len('flow.npy'):30 + len('flow.npy') + len(want)] == want
    assert dn.read_member(path, 'flow', 'cpu') is None                     # no index: the caller falls back to np.load


def test_the_extra_field_round_trips_and_malformed_ones_are_no_index(tmp_path):
    extra = dn.build_extra(4096, [85, 3000, 7000])
    assert dn.parse_extra(extra) == (4096, [85, 3000, 7000])
    other = struct.pack('<HH', 0x5455, 5) + b'\x01abcd'                    # somebody else's field in front
    assert dn.parse_extra(other + extra) == (4096, [85, 3000, 7000])
    assert dn.parse_extra(other) is None and dn.parse_extra(b'') is None
    bad = [extra[:-2],                                                     # cut short
           extra[:4] + struct.pack('<H', 9) + extra[6:],                   # another version
           extra[:8] + struct.pack('<I', 5000) + extra[12:],               # chunk_bytes no power of two
           extra[:12] + struct.pack('<I', 4) + extra[16:],                 # count that does not match the size
           dn.build_extra(4096, [85, 7000, 3000]),                         # offsets not ascending
           struct.pack('<HH', dn.EXTRA_ID, 2) + b'\x01\x00',               # too short for its own header
           struct.pack('<HH', dn.EXTRA_ID, 400) + b'\x01\x00']             # size past the end
    for e in bad:
        assert dn.parse_extra(e) is None
    # a file whose member carries a malformed index: read_member reports "no index" before it touches a device
    arr, C = ARRAYS["field_4096"]
    member, _ = oracle_member('flow', arr, C)
    for k, e in enumerate(bad[:5]):
        path = str(tmp_path / f"m{k}.npz")
        cm.write_npz(path, {'flow': member._replace(extra=e)}, mode='huffman')
        assert dn.read_member(path, 'flow', 'cpu') is None
        if k:                                  # (a field cut short is no zip extra field at all: zipfile refuses the file)
            with np.load(path) as z:
                assert z['flow'].tobytes() == arr.tobytes()
    assert dn.read_member(str(tmp_path / "m0.npz"), 'absent', 'cpu') is None
    assert dn.max_chunks() >= 16000                                        # the library's limit fits the field


def test_an_index_of_hundreds_of_bytes_in_both_headers_loads(tmp_path):
    """400 bytes of extra field here (a 1080p field's 507 chunks make 2 KB) in the local and the central header: np.load
    and zipfile accept it, and find_member reads it back."""
    arr, C = ARRAYS["field_1024"]
    member, _ = oracle_member('flow', arr, C)
    assert len(member.extra) == 16 + 4 * 96
    path = str(tmp_path / "big.npz")
    cm.write_npz(path, {'flow': member}, mode='huffman')
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None and z.getinfo('flow.npy').extra == member.extra
    found = dn.find_member(open(path, 'rb').read(), 'flow')
    assert found is not None and dn.parse_extra(found[4]) == (1024, [len(member.chunks[0]) + o for o in
                                                                       do.deflate(arr.tobytes(), C)[1]])


def test_size_condition_against_the_host_writer():
    """chunk_bytes = 32768 on a seeded 270x480 field: at most 1.005 x the bytes write_npz(mode='huffman') produces for the
    same array (chunking measured +0.022 % at 32 KiB; a block header without run-length symbols costs at most about
    258 x 7 bits per 32 KiB = 0.69 % and far less with short code-length codes)."""
    field = do.flow_field(270, 480, seed=0)
    member, kinds = oracle_member('flow', field, 32768)
    ours = sum(len(c) for c in member.chunks)
    host = cm.host_member('flow', field, 8)
    theirs = sum(len(c) for c in host.chunks)
    print(f"device stream {ours} bytes, host writer {theirs} bytes, ratio {ours / theirs:.5f}, raw {field.nbytes}")
    assert zlib.decompress(b''.join(member.chunks), -15) == dn.npy_head(field.shape) + field.tobytes()
    assert ours <= 1.005 * theirs


# ---- the shared header on the CPU, under sanitizers ---------------------------------------------------------------------
def histograms():
    """(limit, counts) of every chunk of the arrays above, their code-length histograms, and the corner cases."""
    out = []
    for arr, C in ARRAYS.values():
        raw = np.frombuffer(arr.tobytes(), np.uint8)
        for c in range(0, len(raw), C):
            count = np.bincount(raw[c:c + C], minlength=257)
            count[256] = 1
            lit = do.code_lengths(count.tolist(), 15)
            out.append((15, count.tolist()))
            out.append((7, np.bincount(np.asarray(lit + [1, 1]), minlength=19).tolist()))
    out.append((15, [0] * 256 + [1]))                     # one symbol
    out.append((7, [0, 5] + [0] * 17))
    out.append((7, [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 1, 1, 2, 3, 5, 8]))    # deeper than 7
    out.append((15, [1] * 257))
    seen, uniq = set(), []
    for limit, count in out:
        key = (limit, tuple(count))
        if key not in seen:
            seen.add(key)
            uniq.append((limit, count))
    return uniq


def _compilers():
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "video-flow-ml_amd", "vfml", "csrc")]
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
    exe = str(tmp_path_factory.mktemp("deflate_code_host") / "deflate_code_host")
    errors = []
    for cmd in cmds:
        done = subprocess.run([*cmd, os.path.join(ROOT, "tools", "deflate_code_host.cpp"), "-o", exe], capture_output=True,
                              text=True)
        if done.returncode == 0:
            return exe
        errors.append(done.stderr[-600:])
    pytest.fail("tools/deflate_code_host.cpp does not compile with sanitizers:\n" + "\n".join(errors))


def test_the_shared_header_gives_the_oracles_lengths_and_codes(host_program, tmp_path):
    hists = histograms()
    path = str(tmp_path / "hist.txt")
    with open(path, "w") as f:
        for limit, count in hists:
            f.write(f"{limit} {len(count)} " + " ".join(map(str, count)) + "\n")
    done = subprocess.run([host_program, path], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:] + done.stdout[-400:]
    assert "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, done.stderr[-4000:]
    lines = done.stdout.splitlines()
    assert len(lines) == 2 * len(hists) + 2
    for k, (limit, count) in enumerate(hists):
        lens = do.code_lengths(count, limit)
        assert lines[2 * k] == "lens " + " ".join(map(str, lens)), f"histogram {k} (limit {limit})"
        assert lines[2 * k + 1] == "codes " + " ".join(map(str, do.canonical_codes(lens)))
    assert lines[-2] == "pow8 ok"
    assert lines[-1] == f"crc {zlib.crc32(b'123456789'):08x}"


def test_submit_members_writes_the_files_and_members_of_the_host_writer(tmp_path):
    """AsyncFlowCacheWriter.submit_members (finished streams: here the oracle's in the device's place) against submit
    (arrays): the same files, member names, dtypes, shapes and values, with and without LOD files."""
    from storage.async_writer import AsyncFlowCacheWriter
    from storage.cache_manager import LODGenerator
    field = do.flow_field(45, 70, seed=9)
    for num_lods in (0, 5):
        a, b = str(tmp_path / f"streams{num_lods}"), str(tmp_path / f"arrays{num_lods}")
        levels = LODGenerator.generate_lods(field, 5) if num_lods else [field]
        with AsyncFlowCacheWriter(a, 'npz', workers=2, num_lods=num_lods) as w:
            w.submit_members(4, [(oracle_member('flow', lvl, 1024)[0], lvl.shape) for lvl in levels])
        with AsyncFlowCacheWriter(b, 'npz', workers=2, num_lods=num_lods) as w:
            w.submit(field.copy(), 4, list(levels) if num_lods else None)
        names = sorted(os.listdir(a))
        assert names == sorted(os.listdir(b)) and len(names) == 1 + num_lods
        for name in names:
            with np.load(os.path.join(a, name)) as za, np.load(os.path.join(b, name)) as zb:
                assert list(za.files) == list(zb.files), name
                for m in za.files:
                    assert za[m].dtype == zb[m].dtype and za[m].shape == zb[m].shape and za[m].tobytes() == zb[m].tobytes(), (name, m)
            assert dn.load_indexed(os.path.join(a, name), 'flow') is not None
            assert dn.load_indexed(os.path.join(b, name), 'flow') is None
    with pytest.raises(ValueError):
        with AsyncFlowCacheWriter(str(tmp_path / "flo"), 'flo', workers=1) as w:
            w.submit_members(0, [])
