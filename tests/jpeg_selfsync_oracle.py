"""The self-synchronising entropy decoder's definition in plain Python: the scan cut into
subsequences of S raw bytes, each decoded speculatively, synchronised to the unique fixed point, placed by a prefix sum
of completed blocks, written, and the DC differences summed.  vfml/csrc/jpeg_decode_sync.hip and tools/jpeg_sync_host.cpp
are the same definition in HIP / C++ (vfml/csrc/jpeg_sync_steps.h); this file works differently on purpose - it takes
the stuffing and the markers out of each interval once and maps raw positions onto the rest - so that the two can be
held against each other.  The serial decoder of tests/jpeg_decode_oracle.py is what both must equal.
"""
import bisect

import numpy as np

import jpeg_decode_oracle as jd
from storage import jpeg_parse as jp
from storage import jpeg_tables as jt

ERR_COUNT, ERR_SEQUENCE, ERR_CODE, ERR_INDEX, ERR_DATA = 1, 2, 4, 8, 16
POISON = ("poison",)
_PAD = 16                                   # zero bytes behind an interval: a symbol is at most 31 bits


def serial_coefficients(data):
    """The serial oracle's coefficients [MCUs, 6, 64] (natural order, DC values summed) of a whole file."""
    info = jp.parse(data)
    mrows, cols = info.mcu_grid
    nmcu = mrows * cols
    ri = info.restart_interval or nmcu
    pieces, _ = jd.split_intervals(bytes(data[info.scan[0]:info.scan[1]]), info.intervals)
    tables = [(jd._codes(info.huffman[2 * td]), jd._codes(info.huffman[2 * ta + 1])) for td, ta in info.selectors]
    coef = np.zeros((nmcu, 6, 64), np.int64)
    cnt = dict(stuffed=0, zrl=0, eob_only=0, max_ac_size=0)
    for k, piece in enumerate(pieces):
        jd._decode_interval(piece, min(ri, nmcu - k * ri), tables, coef[k * ri:(k + 1) * ri], cnt)
    return coef


class _Scan:
    """A scan's intervals with stuffing and markers taken out, and the map between raw and remaining bytes."""

    def __init__(self, scan):
        a = np.frombuffer(scan, np.uint8)
        self.a, self.n = a, len(a)
        at = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7)) if len(a) > 1 else np.zeros(0, np.int64)
        self.at = at.tolist()
        self.marks = (a[at + 1] - 0xD0).tolist() if len(at) else []
        self.after = [m + 2 for m in self.at]
        self.start = [0, *self.after]
        self.end = [*self.at, self.n]
        self.rod, self.big, self.total = [], [], []
        for s, e in zip(self.start, self.end):
            seg = a[s:e]
            stuffed = np.zeros(len(seg), bool)
            stuffed[1:] = (seg[1:] == 0) & (seg[:-1] == 0xFF)
            self.rod.append((s + np.flatnonzero(~stuffed)).tolist())
            self.big.append(int.from_bytes(seg[~stuffed].tobytes() + bytes(_PAD), 'big'))
            self.total.append(8 * int((~stuffed).sum()))

    def interval_of(self, byte):
        return bisect.bisect_right(self.after, byte)

    def to_d(self, iv, pos):
        """raw bit position -> bit index in interval iv's remaining bytes (a stuffed byte maps to the byte behind it)"""
        return 8 * bisect.bisect_left(self.rod[iv], pos >> 3) + (pos & 7)

    def to_raw(self, iv, d):
        rod = self.rod[iv]
        return rod[d >> 3] * 8 + (d & 7) if d >> 3 < len(rod) else self.end[iv] * 8 + d - self.total[iv]

    def peek16(self, iv, d):
        return (self.big[iv] >> (self.total[iv] + 8 * _PAD - d - 16)) & 0xFFFF

    def bits(self, iv, d, s):
        return (self.big[iv] >> (self.total[iv] + 8 * _PAD - d - s)) & ((1 << s) - 1)


class _Decoder:
    def __init__(self, data, S):
        if S not in (16, 32, 64, 128, 256, 512, 1024):
            raise ValueError(f"subsequences of {S} bytes: a power of two 16..1024")
        info = jp.parse(data)
        self.info, self.S = info, S
        mrows, cols = info.mcu_grid
        self.nmcu = mrows * cols
        self.ri = info.restart_interval or self.nmcu
        self.sc = _Scan(bytes(data[info.scan[0]:info.scan[1]]))
        self.N = max(1, -(-self.sc.n // S))
        self.tables = [(jd._codes(info.huffman[2 * td]), jd._codes(info.huffman[2 * ta + 1])) for td, ta in info.selectors]
        self.memo = {}
        self.poisoned = 0

    def block0(self, iv):
        return min(iv * self.ri, self.nmcu) * 6

    def speculative(self, i):
        """Subsequence i's entry state before anything is known: block 0, DC next, at its first bit."""
        sc = self.sc
        byte = i * self.S
        iv = sc.interval_of(byte)
        if byte >= sc.end[iv]:                       # on a marker's FF: the decode goes to the marker at once
            return (byte * 8, 0, 0)
        return (sc.to_raw(iv, sc.to_d(iv, byte * 8)), 0, 0)

    def _symbol(self, iv, d, codes):
        v = self.sc.peek16(iv, d)
        for length in range(1, 17):
            sym = codes.get((length, v >> (16 - length)))
            if sym is not None:
                return sym, d + length
        return None, d

    def _extend(self, iv, d, s):
        if s == 0:
            return 0, d
        v = self.sc.bits(iv, d, s)
        return (v if v >= 1 << (s - 1) else v - (1 << s) + 1), d + s

    def decode(self, i, entry, write=False, blk=0, coef=None, touch=None):
        """-> (exit state, blocks completed, interval behind the last marker or -1, error bits)"""
        if not write:
            got = self.memo.get((i, entry))
            if got is not None:
                return got
        sc, S = self.sc, self.S
        lim = min(i * S + S, sc.n)
        last = lim == sc.n
        nmark = len(sc.at)
        poison = entry is POISON
        pos, b, k = (i * S * 8, 0, 0) if poison else entry
        iv = sc.interval_of(pos >> 3)
        d = sc.to_d(iv, pos) if (pos >> 3) < sc.end[iv] else sc.total[iv] + pos - sc.end[iv] * 8
        nblk, mark, err, met_poison = 0, -1, 0, poison
        iend = self.block0(iv + 1)
        for _ in range(9 * S + 31):
            pos = sc.to_raw(iv, d)
            if pos >= lim * 8 and not (write and last):
                break
            marker_here = iv < nmark and sc.at[iv] < lim
            jump = False
            if poison:
                if not marker_here:
                    break
                jump = True
            elif write:
                if blk >= iend:
                    if not marker_here:
                        break
                    jump = True
                elif d > sc.total[iv]:
                    err |= ERR_DATA
                    poison = True
                    continue
            elif iv < nmark and d >= sc.total[iv]:
                jump = True
            if jump:
                iv += 1
                d, b, k, poison, nblk, mark = 0, 0, 0, False, 0, iv
                blk, iend = self.block0(iv), self.block0(iv + 1)
                continue
            comp = 0 if b < 4 else b - 3
            dc, ac = self.tables[comp]
            done = False
            sym, d = self._symbol(iv, d, dc if k == 0 else ac)
            if sym is None:
                err |= ERR_CODE
                poison = met_poison = True
                continue
            if touch is not None:
                touch.add((blk, i))
            if k == 0:
                diff, d = self._extend(iv, d, sym & 15)
                if write:
                    coef[blk // 6, blk % 6, 0] = diff
                k = 1
            else:
                r, s = sym >> 4, sym & 15
                if s == 0:
                    if r != 15:
                        done = True
                    elif k + 16 > 64:
                        err |= ERR_INDEX
                        poison = met_poison = True
                        continue
                    else:
                        k += 16
                else:
                    k += r
                    if k > 63:
                        err |= ERR_INDEX
                        poison = met_poison = True
                        continue
                    val, d = self._extend(iv, d, s)
                    if write:
                        coef[blk // 6, blk % 6, jt.ZIGZAG[k]] = val
                    k += 1
            if done or k >= 64:
                k, b = 0, (b + 1) % 6
                nblk += 1
                blk += 1
                if write and d > sc.total[iv]:
                    err |= ERR_DATA
                    poison = True
        out = (POISON if poison else (sc.to_raw(iv, d), b, k), nblk, mark, err)
        if not write:
            self.memo[(i, entry)] = out
            self.poisoned += met_poison
        return out


def decode(data, S=128):
    """bytes of a JPEG file -> (coef int16 [MCUs, 6, 64] natural order, counters).  counters holds `status` (0 or the
    VFML_JPEG_ERR_* bits) beside the counters of the hard paths."""
    dec = _Decoder(data, S)
    sc, N = dec.sc, dec.N
    cnt = dict(subsequences=N, rounds_max=0, late_sync=0, never_sync=0, straddling_blocks_max=0, split_stuffing=0,
               poisoned=0, markers_inside=0, status=0)
    coef = np.zeros((dec.nmcu, 6, 64), np.int64)
    status = 0
    if len(sc.at) + 1 != dec.info.intervals:
        status |= ERR_COUNT
    if any(m != r % 8 for r, m in enumerate(sc.marks)):
        status |= ERR_SEQUENCE
    if status:
        cnt["status"] = status
        return coef.astype(np.int16), cnt
    a = sc.a
    cnt["split_stuffing"] = sum(1 for i in range(1, N) if a[i * S - 1] == 0xFF and a[i * S] == 0)
    cnt["markers_inside"] = len({m // S for m in sc.at})
    # speculate, then synchronise in rounds: a subsequence is decoded again when the state in front of it changed
    entry = [dec.speculative(i) for i in range(N)]
    rec = [dec.decode(i, entry[i]) for i in range(N)]
    spec_exit = [r[0] for r in rec]
    redecodes = [0] * N
    work = range(1, N)
    for _ in range(N):
        nxt = []
        updates = [(i, rec[i - 1][0]) for i in work if rec[i - 1][0] != entry[i]]
        for i, e in updates:
            entry[i], rec[i] = e, dec.decode(i, e)
            redecodes[i] += 1
            if i + 1 < N:
                nxt.append(i + 1)
        if not updates:
            break
        work = nxt
    assert all(rec[i - 1][0] == entry[i] for i in range(1, N)), "no fixed point within the bound"
    cnt["rounds_max"] = max(redecodes)
    # how far each speculation was from the truth
    known = [r[2] >= 0 for r in rec]                    # a marker inside: the exit state does not depend on the entry
    for j in range(1, N):
        if known[j]:
            continue
        e, at = spec_exit[j], j
        while e != rec[at][0] and at + 1 < N and not known[at + 1]:
            at += 1
            e = dec.decode(at, e)[0]
        if e != rec[at][0]:
            cnt["never_sync"] += 1
        elif at - j >= 2:
            cnt["late_sync"] += 1
    # place and write
    carry, touch = 0, set()
    for i in range(N):
        _, _, _, err = dec.decode(i, entry[i], write=True, blk=carry, coef=coef, touch=touch)
        status |= err
        nblk, mark = rec[i][1], rec[i][2]
        carry = (dec.block0(mark) if mark >= 0 else carry) + nblk
    per_block = {}
    for blk, _ in touch:
        per_block[blk] = per_block.get(blk, 0) + 1
    cnt["straddling_blocks_max"] = max(per_block.values(), default=0)
    cnt["poisoned"] = dec.poisoned
    # DC: inclusive sums of the differences per component, restarted at every interval, the low 16 bits kept
    for m0 in range(0, dec.nmcu, dec.ri):
        part = coef[m0:m0 + dec.ri]
        part[:, :4, 0] = np.cumsum(part[:, :4, 0].reshape(-1)).reshape(-1, 4)
        part[:, 4, 0] = np.cumsum(part[:, 4, 0])
        part[:, 5, 0] = np.cumsum(part[:, 5, 0])
    cnt["status"] = status
    return coef.astype(np.int16), cnt
