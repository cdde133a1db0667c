"""The project's baseline JPEG restated in numpy: the integer definition that vfml/csrc/jpeg.hip
implements, byte for byte.  8-bit, YCbCr 4:2:0, the Annex K tables unoptimised, one MCU row per restart interval.
Tables and marker segments come from storage/jpeg_tables.py (test_jpeg_cpu.py holds those to a Pillow-written file).
"""
import numpy as np

from storage import jpeg_tables as jt

_C = jt.dct_matrix()
_ZZ = np.array(jt.ZIGZAG)
_CODES = [jt.huffman_codes(t) for t in jt.HUFFMAN]       # DC0, AC0, DC1, AC1


def planes(rgb):
    """RGB uint8 [h,w,3] -> (Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2]) int64, H and W the sides padded to 16 by edge
    replication."""
    h, w = rgb.shape[:2]
    H, W = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    p = np.pad(np.asarray(rgb, dtype=np.int64), ((0, H - h), (0, W - w), (0, 0)), mode='edge')
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16

    def box(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    return y, box(cb), box(cr)


def quantised_blocks(plane, q):
    """int64 plane [8a, 8b] -> quantised coefficients [a, b, 64] in zigzag order (AC clamped to +-1023)."""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(a, 8, b, 8).transpose(0, 2, 1, 3) - 128
    t = (np.einsum('km,abmn->abkn', _C, x) + 1024) >> 11
    y = (np.einsum('abkn,ln->abkl', t, _C) + 16384) >> 15
    assert np.abs(y).max(initial=0) < 2 ** 31
    qq = np.asarray(q, dtype=np.int64).reshape(8, 8)
    v = np.sign(y) * ((np.abs(y) + (qq >> 1)) // qq)
    v = v.reshape(a, b, 64)[..., _ZZ]
    v[..., 1:] = np.clip(v[..., 1:], -1023, 1023)
    return v


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def flush(self):
        """The interval's bytes: padded with 1-bits, FF followed by 00.  -> (bytes, stuffed count)"""
        pad = -self.n % 8
        acc, n = (self.acc << pad) | ((1 << pad) - 1), self.n + pad
        raw = acc.to_bytes(n // 8, 'big')
        self.acc, self.n = 0, 0
        return raw.replace(b'\xff', b'\xff\x00'), raw.count(b'\xff')


def _size(v):
    return int(abs(v)).bit_length()


def _value_bits(v, s):
    return v if v >= 0 else v + (1 << s) - 1


def encode_scan(rgb, quality=95, counters=None):
    """The entropy-coded scan (between SOS and EOI) of an RGB uint8 picture.  counters: a dict that receives
    rst (markers written), stuffed (FF 00 pairs), zrl (ZRL codes), long_runs (zero runs above 15), eob_only (blocks with no AC coefficient),
    max_ac_size."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    q = jt.quant_tables(quality)
    y, cb, cr = planes(rgb)
    by, bcb, bcr = quantised_blocks(y, q[0]), quantised_blocks(cb, q[1]), quantised_blocks(cr, q[1])
    rows, cols = bcb.shape[:2]
    cnt = dict(rst=0, stuffed=0, zrl=0, long_runs=0, eob_only=0, max_ac_size=0)
    out = bytearray()
    for r in range(rows):
        bits = _Bits()
        pred = [0, 0, 0]
        for c in range(cols):
            for comp, blk in ((0, by[2 * r, 2 * c]), (0, by[2 * r, 2 * c + 1]), (0, by[2 * r + 1, 2 * c]),
                              (0, by[2 * r + 1, 2 * c + 1]), (1, bcb[r, c]), (2, bcr[r, c])):
                dc_codes, ac_codes = (_CODES[0], _CODES[1]) if comp == 0 else (_CODES[2], _CODES[3])
                blk = [int(v) for v in blk]
                diff = max(-2047, min(2047, blk[0] - pred[comp]))
                pred[comp] = blk[0]
                s = _size(diff)
                bits.put(*dc_codes[s])
                bits.put(_value_bits(diff, s), s)
                last = 0
                nz = [k for k in range(1, 64) if blk[k]]
                if not nz:
                    cnt['eob_only'] += 1
                for k in nz:
                    run = k - last - 1
                    cnt['long_runs'] += run > 15
                    for _ in range(run >> 4):
                        bits.put(*ac_codes[0xF0])
                        cnt['zrl'] += 1
                    s = _size(blk[k])
                    cnt['max_ac_size'] = max(cnt['max_ac_size'], s)
                    bits.put(*ac_codes[(run & 15) << 4 | s])
                    bits.put(_value_bits(blk[k], s), s)
                    last = k
                if last != 63:
                    bits.put(*ac_codes[0x00])
        data, stuffed = bits.flush()
        cnt['stuffed'] += stuffed
        out += data
        if r != rows - 1:
            out += bytes([0xFF, 0xD0 + (r & 7)])
            cnt['rst'] += 1
    if counters is not None:
        counters.update(cnt)
    return bytes(out)


def encode(rgb, quality=95, counters=None):
    """The whole JPEG file of an RGB uint8 picture."""
    h, w = np.asarray(rgb).shape[:2]
    return jt.jpeg_file(jt.jpeg_header(h, w, quality), encode_scan(rgb, quality, counters))


def pictures():
    """name -> RGB uint8 picture: the cases of the CPU and GPU tests."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:48, 0:64]
    grad = np.stack([xx * 3, yy * 4, (xx + yy) * 2], axis=-1).astype(np.uint8)   # test_avi_writer_mjpg's frame 0
    yy, xx = np.mgrid[0:150, 0:40]
    freq = 128 + 100 * np.cos((2 * (xx % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (yy % 8) + 1) * 7 * np.pi / 16)
    return {
        "gradient48x64": grad,
        "random45x67": rng.integers(0, 256, (45, 67, 3), dtype=np.uint8),
        "one1x1": np.array([[[200, 30, 90]]], dtype=np.uint8),
        "smooth16x16": np.stack([np.add.outer(np.arange(16) * 9, np.arange(16) * 6)] * 3, axis=-1).astype(np.uint8),
        "binary33x17": (rng.integers(0, 2, (33, 17, 3)) * 255).astype(np.uint8),
        "noise150x40": rng.integers(0, 256, (150, 40, 3), dtype=np.uint8),
        "checker150x40": np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1),
        "flat150x40": np.full((150, 40, 3), (90, 140, 200), dtype=np.uint8),
        # (cast by truncation: 28..228, no clipping needed)
        "frequency150x40": np.repeat(freq.astype(np.uint8)[..., None], 3, axis=-1),
    }
