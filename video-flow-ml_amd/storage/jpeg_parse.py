"""The marker segments of a JPEG file, read on the host for the device decoder (vfml_jpeg_decode_rgb, DESIGN.md
section 13).  Pure Python, no Pillow; only the segments in front of the scan are looked at, the entropy-coded data is
located, never read.

Accepted: baseline sequential DCT (SOF0), 8-bit samples, three components sampled 2x2 / 1x1 / 1x1 in one interleaved
scan - with parse(data, DEVICE_SAMPLINGS) also 2x1 / 1x1 / 1x1 (4:2:2), 1x1 / 1x1 / 1x1 (4:4:4) and one component
(grey, any factors) - 8-bit quantisation tables, Huffman tables from the file (a file without DHT gets the T.81 Annex
K tables of storage/jpeg_tables.py, the MJPG "AVI1" convention), any restart interval.  APPn and COM are skipped.
Anything else raises JpegUnsupported with a message that names it.
"""
from dataclasses import dataclass

import numpy as np

from . import jpeg_tables as jt


class JpegUnsupported(ValueError):
    """The file is a kind of JPEG the device decoder does not take (or no JPEG at all)."""


@dataclass
class JpegInfo:
    h: int
    w: int
    qtables: np.ndarray          # uint8 [3, 64]: the quantisation table of Y, Cb, Cr, natural (row-major) order (grey: Y's x 3)
    huffman: tuple               # (BITS, HUFFVAL) of DC0, AC0, DC1, AC1 (None: not in the file and not used)
    selectors: tuple             # ((dc, ac) table id of Y, of Cb, of Cr); grey: of Y alone
    restart_interval: int        # Ri in MCUs, 0: the scan is one interval
    scan: tuple                  # (start, end) of the entropy-coded data in the file's bytes
    annex_k: bool                # the file holds no DHT segment: the Annex K tables were supplied
    sampling: str = "4:2:0"      # one of DEVICE_SAMPLINGS

    @property
    def mcu_grid(self):
        return jt.mcu_grid(self.h, self.w, self.sampling)

    @property
    def intervals(self):
        rows, cols = self.mcu_grid
        return -(-rows * cols // self.restart_interval) if self.restart_interval else 1


_SOF_NAMES = {0xC1: "extended sequential DCT (SOF1)", 0xC2: "progressive DCT (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential DCT (SOF5)", 0xC6: "differential progressive DCT (SOF6)",
              0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding (SOF10)",
              0xCB: "arithmetic coding (SOF11)", 0xCD: "arithmetic coding (SOF13)", 0xCE: "arithmetic coding (SOF14)",
              0xCF: "arithmetic coding (SOF15)", 0xCC: "arithmetic coding (DAC)"}
_NATURAL = np.array(jt.ZIGZAG)
DEVICE_SAMPLINGS = ("4:2:0", "4:2:2", "4:4:4", "grey")      # what the device kernels take
_FACTORS = {(0x22, 0x11, 0x11): "4:2:0", (0x21, 0x11, 0x11): "4:2:2", (0x11, 0x11, 0x11): "4:4:4"}
_FACTOR_TEXT = {"4:2:0": "2x2 / 1x1 / 1x1 (4:2:0)", "4:2:2": "2x1 / 1x1 / 1x1 (4:2:2)", "4:4:4": "1x1 / 1x1 / 1x1 (4:4:4)"}


def _check_huffman(bits, vals, what):
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > 1 << length:
            raise JpegUnsupported(f"JPEG: {what} is no prefix code (too many codes of {length} bits)")
        code <<= 1
    if len(vals) != sum(bits) or len(vals) > 256:
        raise JpegUnsupported(f"JPEG: {what} holds {len(vals)} symbols for {sum(bits)} codes")


def parse(data, samplings=("4:2:0",)):
    """bytes of a JPEG file -> JpegInfo; JpegUnsupported for anything the device decoder does not take.  samplings: the
    kinds of frame the caller takes, of DEVICE_SAMPLINGS; a file of another kind is refused."""
    samplings = tuple(samplings)
    colour = [s for s in DEVICE_SAMPLINGS[:3] if s in samplings]
    if not isinstance(data, (bytes, bytearray)):
        data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegUnsupported("JPEG: no SOI marker at the start")
    quant, huff, frame, ri, dht_seen = {}, {}, None, 0, False
    i = 2
    while True:
        if i + 4 > n:
            raise JpegUnsupported("JPEG: the file ends before a scan")
        if data[i] != 0xFF:
            raise JpegUnsupported(f"JPEG: byte {data[i]:#04x} at {i} where a marker should be")
        m = data[i + 1]
        if m == 0xFF:                       # fill byte
            i += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:  # stand-alone markers
            i += 2
            continue
        if m == 0xD9:
            raise JpegUnsupported("JPEG: EOI before a scan")
        size = (data[i + 2] << 8) | data[i + 3]
        seg = bytes(data[i + 4:i + 2 + size])
        if size < 2 or i + 2 + size > n:
            raise JpegUnsupported(f"JPEG: segment {m:#04x} at {i} runs past the end of the file")
        i += 2 + size
        if m in _SOF_NAMES:
            raise JpegUnsupported(f"JPEG: {_SOF_NAMES[m]} is not built; baseline sequential DCT (SOF0) only")
        if m == 0xDC:
            raise JpegUnsupported("JPEG: a DNL segment (number of lines defined after the scan) is not built")
        if m == 0xC0:
            if frame is not None:
                raise JpegUnsupported("JPEG: a second frame header")
            if len(seg) < 6:
                raise JpegUnsupported("JPEG: SOF0 segment too short")
            p, h, w, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if p != 8:
                raise JpegUnsupported(f"JPEG: {p}-bit sample precision is not built; 8-bit only")
            if nf != 3 and not (nf == 1 and "grey" in samplings):
                raise JpegUnsupported(f"JPEG: {nf} component(s); three (Y Cb Cr) "
                                      + ("or one (grey) only" if "grey" in samplings else "only"))
            if len(seg) != 6 + 3 * nf:
                raise JpegUnsupported("JPEG: SOF0 segment length does not fit its components")
            if h == 0:
                raise JpegUnsupported("JPEG: zero lines in the frame header (DNL) is not built")
            if w == 0:
                raise JpegUnsupported("JPEG: zero samples per line")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c], seg[8 + 3 * c]) for c in range(nf)]
            factors = tuple(c[1] for c in comps)
            kind = "grey" if nf == 1 else _FACTORS.get(factors)
            if nf == 1:
                if not (1 <= factors[0] >> 4 <= 4 and 1 <= factors[0] & 15 <= 4):
                    raise JpegUnsupported(f"JPEG: sampling factors {factors[0] >> 4}x{factors[0] & 15} outside 1..4")
            elif kind not in samplings:
                said = "JPEG: sampling factors " + " / ".join(f"{s >> 4}x{s & 15}" for s in factors)
                if factors[1] != factors[2] and len(colour) > 1:     # the one-sampling call keeps its wording
                    said += ": chroma components whose factors differ from each other are not built"
                raise JpegUnsupported(said + "; " + ", ".join(_FACTOR_TEXT[s] for s in colour) + " only")
            frame = (h, w, comps, kind)
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    raise JpegUnsupported(f"JPEG: 16-bit quantisation table {tq} is not built; 8-bit tables only")
                if at + 65 > len(seg):
                    raise JpegUnsupported("JPEG: DQT segment too short")
                zz = np.frombuffer(seg, np.uint8, 64, at + 1)
                nat = np.zeros(64, np.uint8)
                nat[_NATURAL] = zz
                quant[tq] = nat
                at += 65
        elif m == 0xC4:
            dht_seen = True
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    raise JpegUnsupported("JPEG: DHT segment too short")
                cls, th = seg[at] >> 4, seg[at] & 15
                bits = tuple(seg[at + 1:at + 17])
                cnt = sum(bits)
                vals = tuple(seg[at + 17:at + 17 + cnt])
                what = f"Huffman table {'AC' if cls else 'DC'}{th}"
                if cls > 1 or th > 1:
                    raise JpegUnsupported(f"JPEG: {what} (class {cls}, id {th}) is outside baseline (ids 0 and 1)")
                _check_huffman(bits, vals, what)
                huff[2 * th + cls] = (bits, vals)
                at += 17 + cnt
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegUnsupported("JPEG: DRI segment length")
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            if frame is None:
                raise JpegUnsupported("JPEG: a scan before the frame header")
            ns = seg[0] if seg else 0
            if ns != len(frame[2]):
                raise JpegUnsupported(f"JPEG: a scan of {ns} component(s): several scans are not built; one "
                                      f"interleaved scan of Y Cb Cr only")
            if len(seg) != 1 + 2 * ns + 3:
                raise JpegUnsupported("JPEG: SOS segment length does not fit its components")
            sel = []
            for c in range(ns):
                cid, tables = seg[1 + 2 * c], seg[2 + 2 * c]
                if cid != frame[2][c][0]:
                    raise JpegUnsupported("JPEG: the scan's components are not in the frame's order Y Cb Cr")
                sel.append((tables >> 4, tables & 15))
            if tuple(seg[1 + 2 * ns:]) != (0, 63, 0):
                raise JpegUnsupported("JPEG: spectral selection / successive approximation in a sequential scan")
            break
        # APPn, COM and anything else with a length: skipped
    h, w, comps, kind = frame
    if not dht_seen:
        huff = {k: t for k, t in enumerate(jt.HUFFMAN)}
    for c, (td, ta) in enumerate(sel):
        if td > 1 or ta > 1 or 2 * td not in huff or 2 * ta + 1 not in huff:
            raise JpegUnsupported(f"JPEG: component {c} uses Huffman tables DC{td} / AC{ta} that the file does not define")
        if comps[c][2] not in quant:
            raise JpegUnsupported(f"JPEG: component {c} uses quantisation table {comps[c][2]} that the file does not define")
    # the scan runs to the first EOI behind its header (FF D9 cannot occur in entropy data); without one, to the end
    end = data.find(jt.EOI, i)
    if end < 0:
        end = n
    return JpegInfo(h=h, w=w, qtables=np.stack([quant[c[2]] for c in (comps * 3)[:3]]),
                    huffman=tuple(huff.get(k) for k in range(4)), selectors=tuple(sel), restart_interval=ri,
                    scan=(i, end), annex_k=not dht_seen, sampling=kind)


def huffman_lookup(table):
    """(BITS, HUFFVAL) -> (limit[16], offset[16]): a code of length l (1..16) is the first l for which the next 16
    bits v of the stream, as a number, are below limit[l-1]; its symbol is HUFFVAL[offset[l-1] + (v >> (16 - l))].
    v at or above limit[15] is a code that is in no table."""
    limit, offset = [0] * 16, [0] * 16
    if table is None:
        return limit, offset
    bits, _ = table
    code = k = 0
    for length in range(1, 17):
        offset[length - 1] = k - code
        code += bits[length - 1]
        k += bits[length - 1]
        limit[length - 1] = code << (16 - length)
        code <<= 1
    return limit, offset


def decode_plan(info):
    """The device kernel a file gets: 'interval' - one restart interval per wave - when an
    interval holds at most one MCU row of MCUs, as in this project's own files; 'sync' - the self-synchronising decoder,
    one lane per subsequence of the scan - when it holds more: Ri = 0 (Pillow, OpenCV, ffmpeg) or Ri above a row."""
    ri = info.restart_interval
    return "sync" if ri == 0 or ri > info.mcu_grid[1] else "interval"


TABLE_INTS = 8 + 4 * 96
SAMPLING_CODE = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2, "grey": 3}      # VFML_JPEG_* of include/vfml.h


def decode_tables(info):
    """-> (qtables uint8 [3,64], tables int32 [392]): what vfml_jpeg_decode_rgb_sampled reads (layout in include/vfml.h):
    tables[2c], tables[2c+1] = index (0..3, in the order DC0 AC0 DC1 AC1) of component c's DC and AC table; from
    tables[8] on, per table 96 ints: limit[16], offset[16] (huffman_lookup) and HUFFVAL as 256 bytes."""
    t = np.zeros(TABLE_INTS, np.int32)
    for c, (td, ta) in enumerate((info.selectors * 3)[:3]):      # grey: the unused entries hold Y's
        t[2 * c], t[2 * c + 1] = 2 * td, 2 * ta + 1
    for k, table in enumerate(info.huffman):
        limit, offset = huffman_lookup(table)
        base = 8 + 96 * k
        t[base:base + 16] = limit
        t[base + 16:base + 32] = offset
        if table is not None:
            vals = np.zeros(256, np.uint8)
            vals[:len(table[1])] = table[1]
            t[base + 32:base + 96] = vals.view(np.int32)
    return np.ascontiguousarray(info.qtables, dtype=np.uint8), t
