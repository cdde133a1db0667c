"""vfml_deflate_huffman and vfml_inflate_chunks on the MI355X against the numpy oracle (tests/deflate_oracle.py): the
encoder byte for byte (stream, chunk offsets, length, CRC) over the edge lengths and histograms, guard bytes and a short
capacity; the inflater over the oracle's streams, the device's own, zlib's fixed and stored blocks, and the damaged
streams (status bit and guard bytes).  Small chunks throughout: nothing here takes more than a second or two."""
import functools
import zlib

import numpy as np
import pytest
import torch

import deflate_oracle as do

pytestmark = pytest.mark.gpu

FIELD = do.flow_field(96, 128, seed=3).tobytes()


def _rng_bytes(seed, n, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def case_bytes(name, C):
    if name.startswith("len"):
        n = {"len1": 1, "lenC-1": C - 1, "lenC": C, "lenC+1": C + 1, "len3C+17": 3 * C + 17}[name]
        return FIELD[:n]
    if name == "field":
        return FIELD
    if name == "constant":
        return bytes([7]) * (2 * C + 5)
    if name == "two_symbols":
        return bytes(np.where(np.frombuffer(_rng_bytes(1, 2 * C + 3), np.uint8) < 70, 65, 200).astype(np.uint8))
    if name == "all256_equal":
        return np.random.default_rng(2).permutation(np.tile(np.arange(256, dtype=np.uint8), 2 * C // 256)).tobytes()
    if name == "uniform_random":
        return _rng_bytes(4, 3 * C + 1)
    if name == "fibonacci":
        return do.fibonacci_chunk()
    if name == "deep":
        return do.deep_chunk()
    raise KeyError(name)


CASES = [(n, C) for C in (1024, 4096) for n in ("len1", "lenC-1", "lenC", "lenC+1", "len3C+17", "field", "constant",
                                                 "two_symbols", "all256_equal", "uniform_random")]
CASES += [("fibonacci", 4096), ("deep", 8192)]
IDS = [f"{n}-{C}" for n, C in CASES]


@functools.lru_cache(maxsize=None)
def oracle(name, C, crc_init=0):
    raw = case_bytes(name, C)
    stream, offsets, crc, kinds = do.deflate(raw, C, crc_init)
    assert zlib.decompress(stream, -15) == raw and crc == zlib.crc32(raw, crc_init)
    return raw, stream, offsets, crc, kinds


def to_dev(gpu, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(gpu)


def device_deflate(gpu, raw, C, crc_init=0, **kw):
    from vfml import hip
    stream, cells = hip.deflate(to_dev(gpu, raw), C, crc_init, **kw)
    assert cells.dtype == torch.int32 and cells.is_cuda
    return hip.deflate_stream(stream, cells)


@pytest.mark.parametrize("name,C", CASES, ids=IDS)
def test_encoder_equals_the_oracle(gpu, name, C):
    raw, stream, offsets, crc, kinds = oracle(name, C)
    got, got_crc, got_offsets = device_deflate(gpu, raw, C)
    assert got_offsets == offsets
    assert len(got) == len(stream)
    assert got == stream, f"first difference at byte {next(i for i in range(len(stream)) if got[i] != stream[i])}"
    assert got_crc == crc


def test_the_cases_take_the_paths_they_are_meant_to():
    assert set(oracle("uniform_random", 1024)[4]) == {"stored"}
    assert set(oracle("field", 4096)[4]) == {"dynamic"}
    count = np.bincount(np.frombuffer(do.deep_chunk(), np.uint8), minlength=257)
    count[256] = 1
    assert max(do.code_lengths(count.tolist(), 40)) > 15 and max(do.code_lengths(count.tolist(), 15)) == 15


def test_crc_continues_from_crc_init(gpu):
    raw, stream, offsets, crc, _ = oracle("len3C+17", 1024, 0x89ABCDEF)
    got, got_crc, got_offsets = device_deflate(gpu, raw, 1024, 0x89ABCDEF)
    assert (got, got_crc, got_offsets) == (stream, crc, offsets)
    assert got_crc == zlib.crc32(raw, 0x89ABCDEF) != zlib.crc32(raw)


@pytest.mark.parametrize("offset", [1, 3])
def test_input_as_a_slice_at_an_odd_byte_offset(gpu, offset):
    from vfml import hip
    raw, stream, offsets, crc, _ = oracle("len3C+17", 1024)
    big = to_dev(gpu, b"\xEE" * offset + raw + b"\xEE" * 9)
    out, cells = hip.deflate(big[offset:offset + len(raw)], 1024)
    assert hip.deflate_stream(out, cells) == (stream, crc, offsets)


@pytest.mark.parametrize("lead", [16, 5])
def test_out_inside_a_larger_buffer_keeps_its_guard_bytes(gpu, lead):
    from vfml import hip
    raw, stream, offsets, crc, _ = oracle("len3C+17", 1024)
    big = torch.full((lead + len(stream) + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    out, cells = hip.deflate(to_dev(gpu, raw), 1024, out=big[lead:lead + len(stream)])
    assert hip.deflate_stream(out, cells) == (stream, crc, offsets)
    host = big.cpu().numpy()
    assert (host[:lead] == 0xA5).all() and (host[lead + len(stream):] == 0xA5).all()


def test_a_capacity_five_bytes_short_reports_the_length_and_writes_nothing_past_it(gpu):
    from vfml import hip
    raw, stream, offsets, crc, _ = oracle("len3C+17", 1024)
    short = len(stream) - 5
    big = torch.full((short + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    out, cells = hip.deflate(to_dev(gpu, raw), 1024, out=big[:short])
    host_cells = [int(v) & 0xFFFFFFFF for v in cells.cpu().tolist()]
    assert host_cells[0] == len(stream) and host_cells[1] == crc and host_cells[2:] == offsets
    host = big.cpu().numpy()
    assert (host[short:] == 0xA5).all()
    assert host[:short].tobytes() == stream[:short]
    with pytest.raises(RuntimeError, match=str(len(stream))):
        hip.deflate_stream(out, cells)


def test_unsupported_sizes(gpu):
    from vfml import hip
    assert hip.deflate_capacity(0) == 0 and hip.deflate_capacity(100, 1000) == 0 and hip.deflate_capacity(100, 65536) == 0
    assert hip.deflate_capacity(16001 * 1024, 1024) == 0 and hip.deflate_capacity(16000 * 1024, 1024) > 0
    with pytest.raises(ValueError):
        hip.deflate(torch.zeros(100, dtype=torch.uint8, device=gpu), 1000)


# ---- inflater -------------------------------------------------------------------------------------------------------
def device_inflate(gpu, stream, offsets, C, raw_bytes, crc_init=0, lead=16):
    """-> (raw bytes, crc, status); the output sits inside a larger buffer whose guard bytes are checked."""
    from vfml import hip
    big = torch.full((lead + raw_bytes + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    data = to_dev(gpu, stream) if len(stream) else torch.empty(0, dtype=torch.uint8, device=gpu)
    out, cells = hip.inflate(data, offsets, C, raw_bytes, crc_init, out=big[lead:lead + raw_bytes])
    host = big.cpu().numpy()
    assert (host[:lead] == 0xA5).all() and (host[lead + raw_bytes:] == 0xA5).all(), "guard bytes around raw were written"
    crc, status = (int(v) & 0xFFFFFFFF for v in cells.cpu().tolist())
    return host[lead:lead + raw_bytes].tobytes(), crc, status


@pytest.mark.parametrize("name,C", CASES, ids=IDS)
def test_inflate_returns_the_input_of_oracle_and_device_streams(gpu, name, C):
    from vfml import hip
    raw, stream, offsets, crc, _ = oracle(name, C)
    assert device_inflate(gpu, stream, offsets, C, len(raw)) == (raw, crc, 0)
    dev_stream, dev_cells = hip.deflate(to_dev(gpu, raw), C)
    n = int(dev_cells[0].item())
    out, cells = hip.inflate(dev_stream[:n], dev_cells[2:], C, len(raw))          # the device's own, never on the host
    assert out.cpu().numpy().tobytes() == raw
    assert hip.inflate_check(cells, crc) == crc


def test_inflate_continues_crc_init(gpu):
    raw, stream, offsets, crc, _ = oracle("len3C+17", 1024, 0x89ABCDEF)
    assert device_inflate(gpu, stream, offsets, 1024, len(raw), 0x89ABCDEF) == (raw, crc, 0)


def zlib_chunks(raw, C):
    """Chunks coded by zlib itself, alternately a fixed-Huffman block (Z_FIXED) and a stored block (level 0), each
    chunk flushed to a byte boundary."""
    out, offsets = [], []
    n = (len(raw) + C - 1) // C
    for c in range(n):
        co = zlib.compressobj(0 if c % 2 else 1, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY if c % 2 else zlib.Z_FIXED)
        piece = co.compress(raw[c * C:(c + 1) * C]) + co.flush(zlib.Z_FINISH if c == n - 1 else zlib.Z_FULL_FLUSH)
        offsets.append(sum(map(len, out)))
        out.append(piece)
    return b"".join(out), offsets


def test_inflate_reads_zlibs_fixed_and_stored_blocks(gpu):
    C = 1024
    # bytes below 144 have 8-bit fixed codes, so zlib keeps the fixed block instead of storing; a few 9-bit ones per chunk
    data = np.frombuffer(_rng_bytes(11, 3 * C + 300, 0, 144), np.uint8).copy()
    data[::211] = 250
    raw = data.tobytes()
    stream, offsets = zlib_chunks(raw, C)
    assert stream[offsets[0]] & 6 == 2 and stream[offsets[1]] & 6 == 0 and stream[offsets[2]] & 6 == 2   # BTYPE 01, 00, 01
    assert do.inflate(stream, offsets, C, len(raw)) == (raw, 0)          # literals only: the seed gives zlib no match
    assert device_inflate(gpu, stream, offsets, C, len(raw)) == (raw, zlib.crc32(raw), 0)


def test_inflate_reads_zlibs_dynamic_blocks_with_run_lengths(gpu):
    C = 4096
    raw = FIELD[:2 * C + 100]
    out, offsets = [], []
    for c in range(3):
        co = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        offsets.append(sum(map(len, out)))
        out.append(co.compress(raw[c * C:(c + 1) * C]) + co.flush(zlib.Z_FINISH if c == 2 else zlib.Z_FULL_FLUSH))
    stream = b"".join(out)
    assert stream[0] & 6 == 4
    assert device_inflate(gpu, stream, offsets, C, len(raw)) == (raw, zlib.crc32(raw), 0)


def damaged():
    C = 1024
    raw, stream, offsets, crc, kinds = oracle("len3C+17", C)
    assert kinds[1] == "dynamic"
    one = oracle("lenC", C)
    assert one[4] == ("dynamic",) or list(one[4]) == ["dynamic"]
    yield "truncated_inside_a_chunk", one[1][:len(one[1]) - 40], one[2], C, do.ERR_BITS
    flipped = bytearray(stream)
    flipped[offsets[1]] ^= 2                      # BTYPE 10 -> 11 in chunk 1's block header
    yield "flipped_header_bit", bytes(flipped), offsets, len(raw), do.ERR_CODE
    yield "offset_past_the_end", stream, offsets[:-1] + [len(stream) + 100], len(raw), do.ERR_CHUNK
    rep = (b"flow cache " * 200)[:C + 50]
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    first = co.compress(rep[:C]) + co.flush(zlib.Z_FULL_FLUSH)
    second = co.compress(rep[C:]) + co.flush()
    yield "zlib_level6_match", first + second, [0, len(first)], len(rep), do.ERR_MATCH
    bad = bytearray(oracle("uniform_random", C)[1])
    bad[3] ^= 0x10                                # NLEN of chunk 0's stored block
    yield "stored_length", bytes(bad), oracle("uniform_random", C)[2], 3 * C + 1, do.ERR_STORED
    longer = do.deflate(raw[:2 * C + 17] + raw[:17], C)        # a last chunk of 34 bytes where 17 are expected
    yield "wrong_length", longer[0], longer[1], 2 * C + 17, do.ERR_LENGTH


DAMAGED = {name: rest for name, *rest in damaged()}


@pytest.mark.parametrize("name", list(DAMAGED))
def test_damaged_streams_set_their_status_bit_and_stay_inside_raw(gpu, name):
    stream, offsets, raw_bytes, bit = DAMAGED[name]
    assert do.inflate(stream, offsets, 1024, raw_bytes)[1] & bit, "the oracle's inflater sees another error"
    _, _, status = device_inflate(gpu, stream, offsets, 1024, raw_bytes)
    assert status & bit, f"status {status}, expected bit {bit}"


# ---- archives and the CLI, end to end ---------------------------------------------------------------------------------
def test_device_member_loads_everywhere_and_read_member_returns_it(gpu, tmp_path):
    import zipfile

    from storage import cache_manager as cm
    from storage import device_npz as dn
    field = do.flow_field(96, 128, seed=3)
    t = torch.from_numpy(field).to(gpu)
    member = dn.device_member('flow', t, 4096)
    stream, offsets, crc, _ = do.deflate(field.tobytes(), 4096, dn.head_crc(field.shape))
    assert member == dn.assemble_member('flow', field.shape, stream, crc, offsets, 4096)
    path = str(tmp_path / "f.npz")
    cm.write_npz(path, {'flow': member, 'frame_idx': 2}, mode='huffman')
    with np.load(path) as z:
        assert z['flow'].dtype == np.float32 and np.array_equal(z['flow'].view(np.uint32), field.view(np.uint32))
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
    back = dn.read_member(path, 'flow', gpu)
    assert back.is_cuda and back.dtype == torch.float32 and tuple(back.shape) == field.shape
    assert np.array_equal(back.cpu().numpy().view(np.uint32), field.view(np.uint32))
    assert dn.read_member(path, 'frame_idx', gpu) is None                  # a host-written member: no index
    damaged = bytearray(open(path, 'rb').read())
    damaged[len(damaged) // 2] ^= 0x40                                     # inside the stream: wrong bytes or a status bit
    open(path, 'wb').write(bytes(damaged))
    with pytest.raises(RuntimeError):
        dn.read_member(path, 'flow', gpu)


@pytest.fixture()
def workdir(tmp_path, monkeypatch):
    from vfml import get_cfg
    from vfml.weights import write_seeded_checkpoint
    write_seeded_checkpoint(str(tmp_path), get_cfg(), seed=0)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("VFML_NPZ_DEFLATE", raising=False)
    return tmp_path


def _run(argv):
    import contextlib
    import io

    import flow_processor as fp
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = fp.main(argv)
    assert rc == 0, out.getvalue()
    return out.getvalue()


# The CLI jobs run on 160x128 frames, the size of the other CLI tests: the engine's four-level correlation pyramid takes no
# frame under 128 rows (96 rows raise "too small for a 4-level correlation pyramid" before anything is computed).  A field
# is five chunks of 32768 bytes; the LOD levels are 80x64 (a chunk and a quarter) down to 10x8 (one short chunk).
def _cache_of(folder):
    (cache,) = [p for p in folder.iterdir() if p.is_dir()]
    return cache


@pytest.mark.parametrize("lods", [False, True], ids=["skip_lods", "lods"])
def test_the_cli_writes_the_host_writers_cache_through_the_device(gpu, workdir, monkeypatch, lods):
    import flow_processor as fp
    from storage import device_npz as dn
    monkeypatch.setattr(fp, "DEVICE_NPZ", True)
    base = ["--input", "synthetic:160x128x6", "--interactive", "--sequence-length", "3", "--device", "cuda"]
    base += [] if lods else ["--skip-lods"]
    a, b = workdir / "device", workdir / "host"
    a.mkdir()
    b.mkdir()
    _run(base + ["--output", str(a)])
    monkeypatch.setenv("VFML_NPZ_DEFLATE", "huffman")
    _run(base + ["--output", str(b)])
    ca, cb = _cache_of(a), _cache_of(b)
    names = sorted(p.name for p in ca.iterdir())
    assert names == sorted(p.name for p in cb.iterdir()) and len(names) == (6 * 6 if lods else 6)
    for name in names:
        with np.load(ca / name) as za, np.load(cb / name) as zb:
            assert list(za.files) == list(zb.files), name
            for m in za.files:
                x, y = za[m], zb[m]
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, m)
        indexed = dn.load_indexed(str(ca / name), 'flow')
        assert indexed is not None and indexed["chunk_bytes"] == 32768, name      # the device wrote it ...
        assert dn.load_indexed(str(cb / name), 'flow') is None                    # ... and the host the other


def test_rendering_through_the_device_reader_gives_the_same_video(gpu, workdir, monkeypatch):
    import flow_processor as fp
    base = ["--input", "synthetic:160x128x6", "--sequence-length", "3", "--device", "cuda", "--skip-lods"]
    a, b, c = workdir / "job", workdir / "device", workdir / "host"
    for d in (a, b, c):
        d.mkdir()
    monkeypatch.setattr(fp, "DEVICE_NPZ", True)
    _run(base + ["--interactive", "--output", str(a)])
    cache = _cache_of(a)
    seen = []
    real = fp._FieldReader.get
    monkeypatch.setattr(fp._FieldReader, "get", lambda self, i: seen.append(real(self, i)) or seen[-1])
    _run(base + ["--uncompressed", "--use-flow-cache", str(cache), "--output", str(b)])
    assert len(seen) == 6 and all(torch.is_tensor(f) and f.is_cuda for f in seen)     # inflated on the device
    seen.clear()
    monkeypatch.setattr(fp, "DEVICE_NPZ", False)
    _run(base + ["--uncompressed", "--use-flow-cache", str(cache), "--output", str(c)])
    assert len(seen) == 6 and all(isinstance(f, np.ndarray) for f in seen)
    (vb,) = [p for p in b.iterdir() if p.suffix == ".avi"]
    (vc,) = [p for p in c.iterdir() if p.suffix == ".avi"]
    assert vb.read_bytes() == vc.read_bytes()
