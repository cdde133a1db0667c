"""The device JPEG decoder's definition restated in numpy: baseline sequential DCT, 8-bit,
YCbCr 4:2:0 in one interleaved scan, decoded with T.81 F.2.2 entropy decoding, libjpeg's `jidctint` "islow" inverse
DCT, its h2v2 "fancy" chroma upsampling and its colour conversion - all integer, so the picture equals Pillow's decode
of the same file byte for byte (tests/test_jpeg_decode_cpu.py holds it to that).  vfml/csrc/jpeg_decode.hip is the
same definition in HIP; the marker segments are read by storage/jpeg_parse.py for both.
"""
import numpy as np

from storage import jpeg_parse as jp
from storage import jpeg_tables as jt

_ZZ = np.array(jt.ZIGZAG)


class JpegError(ValueError):
    """A damaged entropy-coded scan: a code in no table, a coefficient index past 63, an interval that runs out of bits,
    a wrong interval count or restart-marker sequence."""


def split_intervals(scan, expected):
    """The scan's bytes -> the byte strings of its restart intervals (markers removed).  JpegError unless there are
    `expected` of them and the markers run RST0, RST1, ... modulo 8.  -> (pieces, wrap-arounds past RST7)"""
    a = np.frombuffer(scan, np.uint8)
    at = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7)) if len(a) > 1 else np.zeros(0, np.int64)
    if len(at) + 1 != expected:
        raise JpegError(f"{len(at) + 1} restart intervals in the scan, the header asks for {expected}")
    marks = a[at + 1] - 0xD0
    if np.any(marks != np.arange(len(at)) % 8):
        raise JpegError("restart markers out of sequence")
    edges = [0, *(at + 2).tolist()]
    ends = [*at.tolist(), len(a)]
    return [bytes(scan[s:e]) for s, e in zip(edges, ends)], max(0, (len(at) - 1) // 8)


def _codes(table):
    """(BITS, HUFFVAL) -> {(length, code): symbol}"""
    return {} if table is None else {(ln, code): sym for sym, (code, ln) in jt.huffman_codes(table).items()}


class _Reader:
    """Bits of one interval, most significant first, FF 00 taken as FF."""

    def __init__(self, raw):
        data = raw.replace(b'\xff\x00', b'\xff')
        self.stuffed = len(raw) - len(data)
        self.total = 8 * len(data)
        self.buf = data + bytes(8)
        self.pos = 0

    def peek16(self):
        p = self.pos >> 3
        return (int.from_bytes(self.buf[p:p + 3], 'big') >> (8 - (self.pos & 7))) & 0xFFFF

    def symbol(self, codes):
        if self.pos > self.total:
            raise JpegError("the interval's bits ran out before its MCUs did")
        v = self.peek16()
        for length in range(1, 17):
            sym = codes.get((length, v >> (16 - length)))
            if sym is not None:
                self.pos += length
                return sym
        raise JpegError("a code that is in no Huffman table")

    def receive_extend(self, s):
        """T.81 F.2.2.1 EXTEND of the next s bits."""
        if s == 0:
            return 0
        p = self.pos >> 3
        v = (int.from_bytes(self.buf[p:p + 4], 'big') >> (32 - (self.pos & 7) - s)) & ((1 << s) - 1)
        self.pos += s
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def _decode_interval(raw, nmcu, tables, out, cnt):
    """raw bytes of one interval -> out [nmcu, 6, 64] coefficients in natural order."""
    rd = _Reader(raw)
    cnt["stuffed"] += rd.stuffed
    pred = [0, 0, 0]
    for m in range(nmcu):
        for b in range(6):
            comp = 0 if b < 4 else b - 3
            dc, ac = tables[comp]
            s = rd.symbol(dc) & 15
            pred[comp] += rd.receive_extend(s)
            out[m, b, 0] = pred[comp]
            k = 1
            while k < 64:
                rs = rd.symbol(ac)
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:                      # EOB
                        cnt["eob_only"] += k == 1
                        break
                    if k + 16 > 64:
                        raise JpegError("a zero run past coefficient 63")
                    cnt["zrl"] += 1
                    k += 16
                    continue
                k += r
                if k > 63:
                    raise JpegError("a coefficient index past 63")
                cnt["max_ac_size"] = max(cnt["max_ac_size"], s)
                out[m, b, _ZZ[k]] = rd.receive_extend(s)
                k += 1
            if rd.pos > rd.total:
                raise JpegError("the interval's bits ran out before its MCUs did")


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _butterfly(i):
    """libjpeg jidctint's 1-D pass on the last axis (8 values), without the final descale."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (i[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = i7, i5, i3, i1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    return np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d], axis=-1)


def idct_blocks(coef, q):
    """coef [..., 64] natural order, q [64] -> samples [..., 8, 8] uint8-valued int64."""
    x = (coef.astype(np.int64) * np.asarray(q, np.int64)).reshape(*coef.shape[:-1], 8, 8)
    ws = _descale(_butterfly(x.swapaxes(-1, -2)), 11).swapaxes(-1, -2)        # pass 1: columns
    return np.clip(_descale(_butterfly(ws), 18) + 128, 0, 255)                # pass 2: rows


def upsample_fancy(c):
    """libjpeg's h2v2 triangle filter: plane [ch, cw] -> [2 ch, 2 cw]."""
    c = c.astype(np.int64)
    ch, cw = c.shape
    r = np.arange(ch)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for parity, nb in ((0, np.maximum(r - 1, 0)), (1, np.minimum(r + 1, ch - 1))):
        s = 3 * c + c[nb]
        left = s[:, np.maximum(np.arange(cw) - 1, 0)]
        right = s[:, np.minimum(np.arange(cw) + 1, cw - 1)]
        out[parity::2, 0::2] = (3 * s + left + 8) >> 4
        out[parity::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def window_intervals(info, rows):
    """-> (first, last + 1) of the restart intervals that rows=(y0, y1) needs: the intervals of its luma rows and of
    chroma rows (y0 >> 1) - 1 .. ((y1 - 1) >> 1) + 1, when Ri is a positive multiple of the MCUs per MCU row; every
    interval otherwise."""
    mrows, cols = info.mcu_grid
    ri = info.restart_interval
    if rows is None or ri == 0 or ri % cols:
        return 0, info.intervals
    y0, y1 = rows
    ch = (info.h + 1) // 2
    c0, c1 = max((y0 >> 1) - 1, 0), min(((y1 - 1) >> 1) + 1, ch - 1)
    m0, m1 = min(y0 // 16, c0 // 8), max((y1 - 1) // 16, c1 // 8)
    k = ri // cols
    return m0 // k, m1 // k + 1


def decode(data, rows=None, counters=None):
    """bytes of a JPEG file -> RGB uint8 [h,w,3]; rows=(y0, y1): rows y0 <= y < y1 of it, from the intervals that hold
    them alone.  counters: a dict that receives intervals, intervals_decoded, rst_wraps (times the marker number went
    past RST7), stuffed (FF 00 pairs in the decoded intervals), zrl, eob_only (blocks with no AC coefficient),
    max_ac_size and own_tables (the file's Huffman tables differ from Annex K)."""
    info = jp.parse(data)
    h, w = info.h, info.w
    y0, y1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= y0 < y1 <= h:
        raise ValueError(f"rows {rows!r} of a picture of {h}")
    mrows, cols = info.mcu_grid
    nmcu = mrows * cols
    ri = info.restart_interval or nmcu
    pieces, wraps = split_intervals(bytes(data[info.scan[0]:info.scan[1]]), info.intervals)
    cnt = dict(intervals=len(pieces), intervals_decoded=0, rst_wraps=wraps, stuffed=0, zrl=0, eob_only=0, max_ac_size=0,
               own_tables=tuple(info.huffman) != tuple(jt.HUFFMAN))
    tables = [(_codes(info.huffman[2 * td]), _codes(info.huffman[2 * ta + 1])) for td, ta in info.selectors]
    coef = np.zeros((nmcu, 6, 64), np.int64)
    first, last = window_intervals(info, None if rows is None else (y0, y1))
    try:
        for k in range(first, last):
            _decode_interval(pieces[k], min(ri, nmcu - k * ri), tables, coef[k * ri:(k + 1) * ri], cnt)
            cnt["intervals_decoded"] += 1
    finally:
        if counters is not None:
            counters.update(cnt)
    coef = coef.reshape(mrows, cols, 6, 64)
    luma = idct_blocks(coef[:, :, :4], info.qtables[0]).reshape(mrows, cols, 2, 2, 8, 8)
    y = luma.transpose(0, 2, 4, 1, 3, 5).reshape(mrows * 16, cols * 16)[:h, :w]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    planes = []
    for c in (1, 2):
        p = idct_blocks(coef[:, :, 3 + c], info.qtables[c]).transpose(0, 2, 1, 3).reshape(mrows * 8, cols * 8)
        planes.append(upsample_fancy(p[:ch, :cw])[:h, :w] - 128)
    cb, cr = planes
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16),
                    y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                    y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)[y0:y1]
