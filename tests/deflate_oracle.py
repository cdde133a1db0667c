"""numpy oracle of the flow cache's deflate stream: the definition that vfml_deflate_huffman
must reproduce byte for byte, an inflater of its own, and the CRC-32 arithmetic the device uses.

The stream of a member: [stored block with the .npy header, made by the host] + per chunk of `chunk_bytes` raw bytes one
dynamic-Huffman block of literals (or a stored block when that is not larger), every chunk but the last followed by an
empty stored block (00 00 FF FF after padding), the last with BFINAL = 1.  `deflate` here produces the chunk part only
(what the device produces); storage/device_npz.py puts the header block in front.

Code lengths (the rule of vfml/csrc/deflate_code.h, restated): used symbols ordered by (count, symbol); two-queue
Huffman, the leaf on a tie; depths clamped to the limit; while the Kraft sum exceeds 1, one code leaves the limit and the
longest shorter code is replaced by two codes a bit longer; lengths handed out by rank, the rarest symbol the longest.
"""
import zlib

import numpy as np

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
ERR_CODE, ERR_MATCH, ERR_LENGTH, ERR_BITS, ERR_STORED, ERR_CHUNK = 1, 2, 4, 8, 16, 32
POLY = 0xEDB88320


# ---- code construction ----------------------------------------------------------------------------------------------
def code_lengths(count, limit):
    """[len per symbol] of the rule above for the histogram `count`."""
    n = len(count)
    used = sorted((s for s in range(n) if count[s] > 0), key=lambda s: (int(count[s]), s))
    m = len(used)
    lens = [0] * n
    if m == 0:
        return lens
    bl = [0] * (limit + 1)
    if m == 1:
        bl[1] = 1
    else:
        w = [int(count[s]) for s in used] + [0] * (m - 1)
        parent = [0] * (2 * m - 1)
        leaf, inode = 0, m
        for nxt in range(m, 2 * m - 1):
            pick = []
            for _ in range(2):
                if leaf < m and (inode >= nxt or w[leaf] <= w[inode]):
                    pick.append(leaf)
                    leaf += 1
                else:
                    pick.append(inode)
                    inode += 1
            w[nxt] = w[pick[0]] + w[pick[1]]
            parent[pick[0]] = parent[pick[1]] = nxt
        for r in range(m):
            d, x = 0, r
            while x != 2 * m - 2:
                x = parent[x]
                d += 1
            bl[min(d, limit)] += 1
        total = sum(bl[i] << (limit - i) for i in range(1, limit + 1))
        while total > (1 << limit):
            bl[limit] -= 1
            for i in range(limit - 1, 0, -1):
                if bl[i]:
                    bl[i] -= 1
                    bl[i + 1] += 2
                    break
            total -= 1
    r = 0
    for ln in range(limit, 0, -1):
        for _ in range(bl[ln]):
            lens[used[r]] = ln
            r += 1
    return lens


def canonical_codes(lens):
    """[code per symbol], already bit-reversed for deflate's LSB-first packing (0 for unused symbols)."""
    limit = max(max(lens), 1)
    bl = [0] * (limit + 2)
    for ln in lens:
        if ln:
            bl[ln] += 1
    first, code = [0] * (limit + 1), 0
    for bits in range(1, limit + 1):
        code = (code + (bl[bits - 1] if bits > 1 else 0)) << 1
        first[bits] = code
    out = []
    for ln in lens:
        if ln == 0:
            out.append(0)
            continue
        c = first[ln]
        first[ln] += 1
        out.append(int(format(c, f"0{ln}b")[::-1], 2))
    return out


# ---- CRC ------------------------------------------------------------------------------------------------------------
def gf_mul(a, b):
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def crc_shift(v, nbytes):
    """v * x^(8 nbytes) mod P."""
    p, k = 0x00800000, 0
    while nbytes >> k:
        if (nbytes >> k) & 1:
            v = gf_mul(v, p)
        p = gf_mul(p, p)
        k += 1
    return v


def crc32_table(data, init=0):
    """CRC-32 with the table the device builds, not through zlib (tests compare the two)."""
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ POLY if c & 1 else c >> 1
        table.append(c)
    c = init ^ 0xFFFFFFFF
    for b in bytes(data):
        c = table[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def crc_combine(parts):
    """parts: [(crc of the piece, its length)], the first piece's crc continuing from crc_init, the others from 0."""
    total = 0
    after = sum(n for _, n in parts)
    for c, n in parts:
        after -= n
        total ^= crc_shift(c, after)
    return total


# ---- encoder --------------------------------------------------------------------------------------------------------
def _pack(codes, lens, nbits_total):
    """LSB-first bit string of the (code, len) sequence as bytes (zero padded)."""
    codes = np.asarray(codes, np.uint32)
    lens = np.asarray(lens, np.int64)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lens) else np.zeros(0, np.int64)
    bits = np.zeros((nbits_total + 7) // 8 * 8, np.uint8)
    for j in range(int(lens.max()) if len(lens) else 0):
        m = lens > j
        bits[start[m] + j] = (codes[m] >> j) & 1
    return np.packbits(bits, bitorder='little').tobytes()


def chunk_block(chunk, final):
    """(bytes of one chunk's block(s), 'dynamic' | 'stored')."""
    data = np.frombuffer(bytes(chunk), np.uint8)
    n = len(data)
    count = np.bincount(data, minlength=257).astype(np.int64)
    count[256] = 1
    lit = code_lengths(count, 15)
    lens259 = lit + [1, 1]
    cl_count = np.bincount(np.asarray(lens259), minlength=19)
    cl = code_lengths(cl_count, 7)
    hclen = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
    lit_codes, cl_codes = canonical_codes(lit), canonical_codes(cl)
    seq_c = [1 if final else 0, 2, 0, 1, hclen - 4] + [cl[CL_ORDER[i]] for i in range(hclen)]
    seq_l = [1, 2, 5, 5, 4] + [3] * hclen
    seq_c += [cl_codes[x] for x in lens259]
    seq_l += [cl[x] for x in lens259]
    lit_c, lit_l = np.asarray(lit_codes, np.uint32), np.asarray(lit, np.int64)
    codes = np.concatenate([np.asarray(seq_c, np.uint32), lit_c[data], lit_c[256:257]])
    lens = np.concatenate([np.asarray(seq_l, np.int64), lit_l[data], lit_l[256:257]])
    nbits = int(lens.sum())
    marker = b'' if final else b'\x00\x00\xff\xff'
    if 5 + n <= (nbits + 7) // 8:
        body = bytes([1 if final else 0]) + n.to_bytes(2, 'little') + (n ^ 0xFFFF).to_bytes(2, 'little') + data.tobytes()
        return body + (b'' if final else b'\x00' + marker), 'stored'
    if final:
        return _pack(codes, lens, nbits), 'dynamic'
    # the empty stored block's three header bits (zeros) follow the end-of-block code, then padding
    return _pack(codes, lens, nbits + 3) + marker, 'dynamic'


def deflate(raw, chunk_bytes, crc_init=0):
    """-> (stream bytes, [offset of every chunk], crc32 of raw continuing from crc_init, [kind per chunk])."""
    raw = bytes(raw)
    assert raw and 1024 <= chunk_bytes <= 32768 and chunk_bytes & (chunk_bytes - 1) == 0
    n = (len(raw) + chunk_bytes - 1) // chunk_bytes
    out, offsets, kinds, parts = [], [], [], []
    pos = 0
    for c in range(n):
        piece = raw[c * chunk_bytes:(c + 1) * chunk_bytes]
        blk, kind = chunk_block(piece, c == n - 1)
        offsets.append(pos)
        pos += len(blk)
        out.append(blk)
        kinds.append(kind)
        parts.append((crc32_table(piece, crc_init if c == 0 else 0), len(piece)))
    return b''.join(out), offsets, crc_combine(parts), kinds


# ---- inflater -------------------------------------------------------------------------------------------------------
def _lut(lens):
    """15-bit lookup (sym | len << 9, 0 = no code) of a canonical code, or None if it is over-subscribed."""
    if sum((1 << (15 - ln)) for ln in lens if ln) > (1 << 15):
        return None
    lut = np.zeros(1 << 15, np.int32)
    for s, (ln, code) in enumerate(zip(lens, canonical_codes(list(lens)))):
        if ln:
            lut[code::1 << ln] = s | (ln << 9)
    return lut


def inflate_chunk(buf, want):
    """Decode the blocks of one chunk (bytes) -> (bytes, status bits)."""
    nbits = len(buf) * 8
    bits = np.unpackbits(np.frombuffer(bytes(buf) + b'\0\0\0', np.uint8), bitorder='little').astype(np.int32)
    win = np.zeros(nbits + 8, np.int32)
    for j in range(15):
        win += bits[j:j + nbits + 8] << j
    pos, out = 0, bytearray()

    def take(k):
        nonlocal pos
        if pos + k > nbits:
            raise EOFError
        v = int(win[pos]) & ((1 << k) - 1)
        pos += k
        return v

    try:
        while True:
            if pos % 8 == 0 and pos == nbits:
                break
            final, btype = take(1), take(2)
            if btype == 0:
                pos = (pos + 7) // 8 * 8
                ln, nln = take(8) | take(8) << 8, take(8) | take(8) << 8
                if ln ^ nln != 0xFFFF:
                    return bytes(out), ERR_STORED
                if pos + 8 * ln > nbits:
                    return bytes(out), ERR_BITS
                if len(out) + ln > want:
                    return bytes(out), ERR_LENGTH
                out += bytes(buf[pos // 8:pos // 8 + ln])
                pos += 8 * ln
            elif btype == 3:
                return bytes(out), ERR_CODE
            else:
                if btype == 1:
                    lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                else:
                    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
                    if hlit > 286 or hdist > 30:
                        return bytes(out), ERR_CODE
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[CL_ORDER[i]] = take(3)
                    clut = _lut(cl)
                    if clut is None:
                        return bytes(out), ERR_CODE
                    lens = []
                    while len(lens) < hlit + hdist:
                        e = int(clut[int(win[pos])]) if pos < nbits else 0
                        if e == 0:
                            return bytes(out), ERR_CODE
                        take(e >> 9)
                        s = e & 511
                        if s < 16:
                            lens.append(s)
                        elif s == 16:
                            if not lens:
                                return bytes(out), ERR_CODE
                            lens += [lens[-1]] * (3 + take(2))
                        elif s == 17:
                            lens += [0] * (3 + take(3))
                        else:
                            lens += [0] * (11 + take(7))
                    if len(lens) > hlit + hdist:
                        return bytes(out), ERR_CODE
                    lit = lens[:hlit]
                lut = _lut(lit)
                if lut is None:
                    return bytes(out), ERR_CODE
                while True:
                    e = int(lut[int(win[pos])]) if pos < nbits else 0
                    if e == 0:
                        return bytes(out), (ERR_BITS if pos + 15 > nbits else ERR_CODE)
                    if pos + (e >> 9) > nbits:
                        return bytes(out), ERR_BITS
                    pos += e >> 9
                    s = e & 511
                    if s == 256:
                        break
                    if s > 256:
                        return bytes(out), ERR_MATCH
                    if len(out) >= want:
                        return bytes(out), ERR_LENGTH
                    out.append(s)
            if final:
                break
    except EOFError:
        return bytes(out), ERR_BITS
    return bytes(out), (0 if len(out) == want else ERR_LENGTH)


def inflate(stream, offsets, chunk_bytes, raw_bytes):
    """-> (raw bytes, OR of the chunks' status bits)."""
    out, status = [], 0
    n = len(offsets)
    for c in range(n):
        a, b = offsets[c], (offsets[c + 1] if c + 1 < n else len(stream))
        want = min(chunk_bytes, raw_bytes - c * chunk_bytes)
        if not (0 <= a <= b <= len(stream)) or want < 1:
            status |= ERR_CHUNK
            out.append(b'\0' * max(want, 0))
            continue
        piece, st = inflate_chunk(stream[a:b], want)
        status |= st
        out.append(piece.ljust(want, b'\0')[:want])
    return b''.join(out), status


# ---- test data ------------------------------------------------------------------------------------------------------
def flow_field(h, w, seed=0):
    """A seeded float32 field [h,w,2]: smooth motion of a few px plus 0.05 px noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    u = 3.0 * np.sin(x / 37.0 + 0.3) + 2.0 * np.cos(y / 23.0) + 0.01 * x
    v = 2.5 * np.cos(x / 41.0) - 1.5 * np.sin(y / 29.0 + 0.7) - 0.008 * y
    f = np.stack([u, v], -1).astype(np.float32)
    return (f + rng.normal(0.0, 0.05, f.shape).astype(np.float32)).astype(np.float32)


def fibonacci_chunk():
    """4096 bytes whose counts are the Fibonacci numbers 1, 1, 2, ... 987 (2583 bytes) and one further symbol for the
    rest: an unlimited Huffman code of it is deeper than 15 bits."""
    fib = [1, 1]
    while fib[-1] < 987:
        fib.append(fib[-1] + fib[-2])
    parts = [np.full(c, 10 + i, np.uint8) for i, c in enumerate(fib)]
    parts.append(np.full(4096 - sum(fib), 200, np.uint8))
    data = np.concatenate(parts)
    return np.random.default_rng(5).permutation(data).tobytes()


def selfcheck(raw, chunk_bytes, crc_init=0):
    stream, offsets, crc, _ = deflate(raw, chunk_bytes, crc_init)
    assert zlib.decompress(stream, -15) == bytes(raw)
    assert crc == zlib.crc32(bytes(raw), crc_init)
    return stream, offsets, crc


def deep_chunk():
    """8192 bytes with counts 1, 2, 3, 5, 8, ... 2584 (one 1 only: with the end-of-block symbol's 1 no two weights tie, so
    the two-queue tree is a chain) and one further symbol for the rest: depths reach past 15 and the repair step runs."""
    fib = [1, 2]
    while fib[-1] < 2584:
        fib.append(fib[-1] + fib[-2])
    parts = [np.full(c, 10 + i, np.uint8) for i, c in enumerate(fib)]
    parts.append(np.full(8192 - sum(fib), 200, np.uint8))
    return np.random.default_rng(6).permutation(np.concatenate(parts)).tobytes()
