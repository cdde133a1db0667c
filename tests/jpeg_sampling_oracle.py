"""The device JPEG decoder's definition for every sampling it takes ("Samplings"), in numpy: the
entropy decoding, the inverse DCT and the colour conversion of tests/jpeg_decode_oracle.py, with the two things that
depend on the sampling - the MCU (its size, its blocks in stream order, where a block lands in its plane) and the chroma
filter - written for 4:2:0, 4:2:2, 4:4:4 and one-component (grey) files.  The picture equals Pillow's decode of the same
file byte for byte (tests/test_jpeg_sampling_cpu.py holds it to that), but for 4:2:0 pictures at most 4 pixels wide,
where this definition keeps the triangle filter of jpeg_decode_oracle.py and libjpeg repeats the samples.

    sampling   MCU (h x w)   blocks of an MCU in stream order
    4:2:0      16 x 16       Y00 Y01 Y10 Y11 Cb Cr
    4:2:2       8 x 16       Y0 Y1 Cb Cr
    4:4:4       8 x 8        Y Cb Cr
    grey        8 x 8        Y         (a one-component scan is not interleaved, T.81 A.2.2: whatever factors it names)
"""
import numpy as np

from jpeg_decode_oracle import JpegError, _Reader, _codes, idct_blocks, split_intervals, upsample_fancy
from storage import jpeg_parse as jp
from storage import jpeg_tables as jt

_ZZ = np.array(jt.ZIGZAG)
# sampling -> (luma blocks down, luma blocks across, chroma blocks per component)
GEOMETRY = {"4:2:0": (2, 2, 1), "4:2:2": (1, 2, 1), "4:4:4": (1, 1, 1), "grey": (1, 1, 0)}


def blocks_per_mcu(sampling):
    vs, hs, nc = GEOMETRY[sampling]
    return vs * hs + 2 * nc


def upsample_h2v1(c):
    """libjpeg's h2v1 filter: plane [ch, cw] -> [ch, 2 cw].  The triangle filter where the plane is more than 2 samples
    wide, neighbours clamped at both ends; every sample repeated where it is narrower."""
    c = c.astype(np.int64)
    ch, cw = c.shape
    out = np.empty((ch, 2 * cw), np.int64)
    if cw <= 2:
        out[:, 0::2] = out[:, 1::2] = c
        return out
    left = c[:, np.maximum(np.arange(cw) - 1, 0)]
    right = c[:, np.minimum(np.arange(cw) + 1, cw - 1)]
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out


def _decode_interval(raw, nmcu, ny, tables, out, cnt):
    """raw bytes of one interval -> out [nmcu, nb, 64] coefficients in natural order; the first ny blocks are luma."""
    rd = _Reader(raw)
    cnt["stuffed"] += rd.stuffed
    nb = out.shape[1]
    pred = [0, 0, 0]
    for m in range(nmcu):
        for b in range(nb):
            comp = 0 if b < ny else b - ny + 1
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
                        break
                    if k + 16 > 64:
                        raise JpegError("a zero run past coefficient 63")
                    k += 16
                    continue
                k += r
                if k > 63:
                    raise JpegError("a coefficient index past 63")
                out[m, b, _ZZ[k]] = rd.receive_extend(s)
                k += 1
            if rd.pos > rd.total:
                raise JpegError("the interval's bits ran out before its MCUs did")


def window_intervals(info, rows):
    """-> (first, last + 1) of the restart intervals that rows=(y0, y1) needs, when Ri is a positive multiple of the MCUs
    per MCU row: the intervals of its luma rows and - in 4:2:0 alone, the one sampling with a vertical filter - of chroma
    rows (y0 >> 1) - 1 .. ((y1 - 1) >> 1) + 1.  Every interval otherwise."""
    mrows, cols = info.mcu_grid
    ri = info.restart_interval
    if rows is None or ri == 0 or ri % cols:
        return 0, info.intervals
    y0, y1 = rows
    mh = jt.MCU_SIZE[info.sampling][0]
    m0, m1 = y0 // mh, (y1 - 1) // mh
    if info.sampling == "4:2:0":
        ch = (info.h + 1) // 2
        c0, c1 = max((y0 >> 1) - 1, 0), min(((y1 - 1) >> 1) + 1, ch - 1)
        m0, m1 = min(m0, c0 // 8), max(m1, c1 // 8)
    k = ri // cols
    return m0 // k, m1 // k + 1


def coefficients(data, rows=None, counters=None):
    """-> (JpegInfo, coef int64 [MCUs, nb, 64] natural order) of the intervals rows=(y0, y1) needs (zeros elsewhere)."""
    info = jp.parse(data, jp.DEVICE_SAMPLINGS)
    vs, hs, nc = GEOMETRY[info.sampling]
    ny, nb = vs * hs, vs * hs + 2 * nc
    mrows, cols = info.mcu_grid
    nmcu = mrows * cols
    ri = info.restart_interval or nmcu
    pieces, wraps = split_intervals(bytes(data[info.scan[0]:info.scan[1]]), info.intervals)
    cnt = dict(intervals=len(pieces), intervals_decoded=0, rst_wraps=wraps, stuffed=0)
    tables = [(_codes(info.huffman[2 * td]), _codes(info.huffman[2 * ta + 1])) for td, ta in info.selectors]
    coef = np.zeros((nmcu, nb, 64), np.int64)
    first, last = window_intervals(info, rows)
    try:
        for k in range(first, last):
            _decode_interval(pieces[k], min(ri, nmcu - k * ri), ny, tables, coef[k * ri:(k + 1) * ri], cnt)
            cnt["intervals_decoded"] += 1
    finally:
        if counters is not None:
            counters.update(cnt)
    return info, coef


def decode(data, rows=None, counters=None):
    """bytes of a JPEG file -> RGB uint8 [h,w,3]; rows=(y0, y1): rows y0 <= y < y1 of it, from the intervals that hold
    them alone.  counters: a dict that receives intervals, intervals_decoded, rst_wraps (times the marker number went
    past RST7) and stuffed (FF 00 pairs in the decoded intervals)."""
    info = jp.parse(data, jp.DEVICE_SAMPLINGS)
    h, w = info.h, info.w
    y0, y1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= y0 < y1 <= h:
        raise ValueError(f"rows {rows!r} of a picture of {h}")
    info, coef = coefficients(data, None if rows is None else (y0, y1), counters)
    vs, hs, nc = GEOMETRY[info.sampling]
    ny = vs * hs
    mrows, cols = info.mcu_grid
    coef = coef.reshape(mrows, cols, -1, 64)
    luma = idct_blocks(coef[:, :, :ny], info.qtables[0]).reshape(mrows, cols, vs, hs, 8, 8)
    y = luma.transpose(0, 2, 4, 1, 3, 5).reshape(mrows * 8 * vs, cols * 8 * hs)[:h, :w]
    if not nc:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)[y0:y1]
    ch, cw = -(-h // vs), -(-w // hs)                # ceil(h V / Vmax) x ceil(w H / Hmax)
    planes = []
    for c in (1, 2):
        p = idct_blocks(coef[:, :, ny + c - 1], info.qtables[c]).transpose(0, 2, 1, 3).reshape(mrows * 8, cols * 8)
        p = p[:ch, :cw]
        p = upsample_fancy(p) if (vs, hs) == (2, 2) else upsample_h2v1(p) if hs == 2 else p
        planes.append(p[:h, :w] - 128)
    cb, cr = planes
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16),
                    y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                    y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)[y0:y1]
