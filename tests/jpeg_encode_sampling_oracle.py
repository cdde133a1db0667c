"""The project's baseline JPEG encoder with the sampling as an argument: the integer definition
that vfml_jpeg_encode_rgb_sampled implements, byte for byte.  Colour conversion, DCT, quantisation, clamps, the Annex K
tables, stuffing, padding and the restart markers are those of tests/jpeg_oracle.py, whose helpers are used here; the
sampling sets the MCU, the chroma sample and the block order of the scan:

    4:2:0   MCU 16 x 16   Y00 Y01 Y10 Y11 Cb Cr   chroma = (a + b + c + d + 2) >> 2 over 2 x 2 cells
    4:2:2   MCU  8 x 16   Y0 Y1 Cb Cr             chroma = (a + b + 1) >> 1 over the horizontal pair
    4:4:4   MCU  8 x  8   Y Cb Cr                 chroma = the sample itself

The picture is padded by edge replication to multiples of the MCU, one MCU row is one restart interval, the DC
predictors are per component and zero at the start of each interval.  At "4:2:0" the scan is jpeg_oracle.encode_scan's.
"""
import numpy as np

from jpeg_oracle import _CODES, _Bits, _size, _value_bits, pictures, quantised_blocks  # noqa: F401 (pictures: the cases)
from storage import jpeg_tables as jt

SAMPLINGS = ("4:2:0", "4:2:2", "4:4:4")
# sampling -> (luma blocks down, luma blocks across) of an MCU
LUMA_BLOCKS = {"4:2:0": (2, 2), "4:2:2": (1, 2), "4:4:4": (1, 1)}


def planes(rgb, sampling):
    """RGB uint8 [h,w,3] -> (Y, Cb, Cr) int64, the sides padded to the MCU by edge replication, chroma sampled."""
    if sampling not in SAMPLINGS:
        raise ValueError(f"sampling {sampling!r}; {', '.join(SAMPLINGS)} are defined")
    h, w = rgb.shape[:2]
    mh, mw = jt.MCU_SIZE[sampling]
    H, W = -(-h // mh) * mh, -(-w // mw) * mw
    p = np.pad(np.asarray(rgb, dtype=np.int64), ((0, H - h), (0, W - w), (0, 0)), mode='edge')
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16

    def sample(c):
        if sampling == "4:2:0":
            return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
        if sampling == "4:2:2":
            return (c[:, 0::2] + c[:, 1::2] + 1) >> 1
        return c
    return y, sample(cb), sample(cr)


def encode_scan(rgb, quality=95, sampling="4:2:0", counters=None):
    """The entropy-coded scan (between SOS and EOI) of an RGB uint8 picture.  counters: as jpeg_oracle.encode_scan's."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    q = jt.quant_tables(quality)
    y, cb, cr = planes(rgb, sampling)
    by, bcb, bcr = quantised_blocks(y, q[0]), quantised_blocks(cb, q[1]), quantised_blocks(cr, q[1])
    rows, cols = bcb.shape[:2]
    assert (rows, cols) == jt.mcu_grid(rgb.shape[0], rgb.shape[1], sampling)
    lv, lh = LUMA_BLOCKS[sampling]
    cnt = dict(rst=0, stuffed=0, zrl=0, long_runs=0, eob_only=0, max_ac_size=0)
    out = bytearray()
    for r in range(rows):
        bits = _Bits()
        pred = [0, 0, 0]
        for c in range(cols):
            blocks = [(0, by[lv * r + i, lh * c + j]) for i in range(lv) for j in range(lh)]
            blocks += [(1, bcb[r, c]), (2, bcr[r, c])]
            for comp, blk in blocks:
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


def encode(rgb, quality=95, sampling="4:2:0", counters=None):
    """The whole JPEG file of an RGB uint8 picture."""
    h, w = np.asarray(rgb).shape[:2]
    return jt.jpeg_file(jt.jpeg_header(h, w, quality, sampling), encode_scan(rgb, quality, sampling, counters))


def motion_edge_picture(h=48, w=64, clamp=32.0):
    """The rg8 picture of a flow with one vertical and one horizontal motion edge: u = 20 / -15 px split at x = 29,
    v = -12 / 9 px split at y = 21; R and G hold (f + clamp) / (2 clamp) * 255 rounded to nearest, B is 0 (the layout of
    motion-vectors-rg8; 4 levels are 1 px of flow at clamp 32).  The levels are R 207 / 68 and G 80 / 163."""
    yy, xx = np.mgrid[0:h, 0:w]
    level = lambda f: np.rint((f + clamp) / (2 * clamp) * 255).astype(np.uint8)
    return np.stack([level(np.where(xx < 29, 20.0, -15.0)), level(np.where(yy < 21, -12.0, 9.0)),
                     np.zeros((h, w), np.uint8)], axis=-1)


def motion_edge_error(rgb, decoded):
    """(max, mean, fraction above 2 levels) of the error in the R and G values of a decoded motion_edge_picture."""
    e = np.abs(np.asarray(decoded, dtype=np.int64)[..., :2] - np.asarray(rgb, dtype=np.int64)[..., :2])
    return int(e.max()), float(e.mean()), float((e > 2).mean())
