// The per-subsequence steps of the self-synchronising JPEG entropy decoder, as code that
// compiles for the host and for the device: vfml/csrc/jpeg_decode_sync.hip runs them one lane per subsequence,
// tools/jpeg_sync_host.cpp runs the same phases in series on the CPU (under sanitizers in tests/test_jpeg_selfsync_cpu.py).
// tests/jpeg_selfsync_oracle.py is the definition in Python.
//
// A state at a symbol boundary is (raw bit position, block in MCU b < nb, coefficient index k; k = 0: DC next).  Positions are
// 64-bit and absolute while a subsequence is decoded; a record keeps them relative to the subsequence's edge (8 bits).
// Every loop is bounded by a count: the interval search by 32 halvings, a refill by 8 bytes, the Huffman search by 8
// lengths, a subsequence decode by 9 S + 31 steps (a symbol is at least one bit, a marker at least two bytes).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VFML_JSYNC_HD __host__ __device__ __forceinline__
#else
#define VFML_JSYNC_HD inline
#endif

namespace vfml_jsync {

constexpr uint32_t kPoison = 0xFFFFFFFFu;        // the exit state of a decode that met what no stream holds
constexpr int kTableInts = 8 + 4 * 96;
enum { kErrCount = 1, kErrSequence = 2, kErrCode = 4, kErrIndex = 8, kErrData = 16 };

// The 392-int tables block (include/vfml.h) unpacked, with a first-level table on the next 8 bits in front of the
// limit / offset search.  3672 bytes: in LDS on the device.
struct Tabs {
  uint16_t lut[4][256];                          // length << 8 | symbol of a code of up to 8 bits; 0: a longer code
  int limit[4][16];
  int offset[4][16];
  uint8_t huffval[4][256];
  uint8_t zigzag[64];
  int dc_t[3], ac_t[3];
};
static_assert(sizeof(Tabs) == 3672, "the LDS figures of DESIGN.md section 13.1 follow this size");

struct Ctx {
  const uint8_t* scan;
  uint32_t n;                                    // bytes of the scan
  const uint32_t* mpos;                          // [nmark] offset of the FF of marker r, ascending
  uint32_t nmark;                                // intervals - 1
  int ri, nmcu;                                  // MCUs per interval (the picture's when Ri = 0), MCUs
  int S;                                         // bytes per subsequence, a power of two 16..1024
  int nb, ny;                                    // blocks per MCU (6 / 4 / 3 / 1 by the sampling), luma blocks among them
};

struct Rec {                                     // one subsequence's record
  uint32_t entry, exit;                          // packed states: the one it was decoded from, the one it ended in
  uint32_t nblk;                                 // blocks completed (behind its last marker, when it holds one)
  int32_t mark;                                  // -1, or the interval that begins behind its last marker
};

struct Out {
  uint32_t exit, nblk;
  int32_t mark;
  int err;
};

VFML_JSYNC_HD uint32_t pack_state(int64_t rel, int b, int k) {
  if (rel < 0 || rel > 255) return kPoison;
  return (uint32_t)rel | (uint32_t)b << 8 | (uint32_t)k << 11;
}

// thread `idx` of `stride` fills its share; `zz` is the zigzag order (natural index of the k-th coefficient)
VFML_JSYNC_HD void tabs_fill(Tabs& t, const int* tables, const uint8_t* zz, int idx, int stride) {
  for (int i = idx; i < 4 * 256; i += stride) {
    const int tab = i >> 8, v = (i & 255) << 8;
    const int* base = tables + 8 + 96 * tab;
    uint16_t e = 0;
    for (int l = 1; l <= 8; ++l)
      if (v < base[l - 1]) {
        const uint32_t at = (uint32_t)(base[16 + l - 1] + (v >> (16 - l))) & 255u;
        const uint32_t sym = ((uint32_t)base[32 + (at >> 2)] >> (8 * (at & 3))) & 255u;
        e = (uint16_t)(l << 8 | sym);
        break;
      }
    t.lut[tab][i & 255] = e;
    t.huffval[tab][i & 255] = (uint8_t)(((uint32_t)base[32 + ((i & 255) >> 2)] >> (8 * (i & 3))) & 255u);
  }
  for (int i = idx; i < 64; i += stride) {
    t.limit[i >> 4][i & 15] = tables[8 + 96 * (i >> 4) + (i & 15)];
    t.offset[i >> 4][i & 15] = tables[8 + 96 * (i >> 4) + 16 + (i & 15)];
    t.zigzag[i] = zz[i];
  }
  for (int i = idx; i < 3; i += stride) t.dc_t[i] = tables[2 * i] & 3, t.ac_t[i] = tables[2 * i + 1] & 3;
}

// the interval that the byte at `bytepos` belongs to: the first marker r with mpos[r] + 2 > bytepos
VFML_JSYNC_HD uint32_t interval_of(const Ctx& c, uint32_t bytepos) {
  uint32_t lo = 0, hi = c.nmark;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (c.mpos[mid] + 2u > bytepos) hi = mid; else lo = mid + 1;
  }
  return lo;
}

VFML_JSYNC_HD uint32_t interval_end(const Ctx& c, uint32_t iv, uint32_t floor_) {
  uint32_t e = iv < c.nmark ? c.mpos[iv] : c.n;
  e = e < c.n ? e : c.n;
  return e > floor_ ? e : floor_;
}

VFML_JSYNC_HD int64_t interval_block0(const Ctx& c, uint32_t iv) {
  const int64_t m = (int64_t)iv * c.ri;
  return (m < c.nmcu ? m : c.nmcu) * c.nb;
}

// ---- bits: most significant first, FF 00 taken as FF where it is met, zeros behind the interval's end --------------
struct Rd {
  uint64_t acc;                                  // the next bits
  uint64_t jump;                                 // the first bit of a byte in front of which a stuffed 00 was skipped
  int nb;
  uint32_t q, end, prev;                         // next raw byte, end of the interval, the raw byte before q
  int64_t pos;                                   // raw position of the next bit
};

VFML_JSYNC_HD void rd_fill(Rd& r, const Ctx& c) {
  for (int it = 0; it < 8 && r.nb <= 56; ++it) {
    uint32_t byte = 0;
    uint64_t flag = 0;
    if (r.q < r.end) {
      byte = c.scan[r.q];
      if (byte == 0u && r.prev == 0xFFu) {
        ++r.q, flag = 1;
        byte = r.q < r.end ? c.scan[r.q] : 0u;
      }
    }
    r.prev = byte;
    ++r.q;
    r.acc |= (uint64_t)byte << (56 - r.nb);
    r.jump |= flag << (63 - r.nb);
    r.nb += 8;
  }
  if (r.jump >> 63) r.pos += 8, r.jump &= ~(1ull << 63);      // a position never points at a stuffed byte
}

VFML_JSYNC_HD void rd_take(Rd& r, int l) {                   // l in 1..16
  r.pos += l + 8 * (int)__builtin_popcountll(r.jump >> (64 - l));
  r.acc <<= l, r.jump <<= l, r.nb -= l;
}

VFML_JSYNC_HD void rd_start(Rd& r, const Ctx& c, int64_t pos, uint32_t end) {
  r.acc = 0, r.jump = 0, r.nb = 0, r.end = end, r.pos = pos;
  r.q = (uint32_t)(pos >> 3);
  r.prev = r.q > 0 && r.q <= c.n ? c.scan[r.q - 1] : 0u;
  rd_fill(r, c);
  const int off = (int)(pos & 7);
  r.acc <<= off, r.jump <<= off, r.nb -= off;
}

// -> the symbol, or -1 for a code that is in no table
VFML_JSYNC_HD int rd_symbol(Rd& r, const Tabs& t, int tab) {
  const int v = (int)(r.acc >> 48);
  const uint32_t e = t.lut[tab][v >> 8];
  if (e) {
    rd_take(r, (int)(e >> 8));
    return (int)(e & 255u);
  }
  for (int i = 8; i < 16; ++i)
    if (v < t.limit[tab][i]) {
      const int sym = t.huffval[tab][(uint32_t)(t.offset[tab][i] + (v >> (15 - i))) & 255u];
      rd_take(r, i + 1);
      return sym;
    }
  return -1;
}

VFML_JSYNC_HD int rd_extend(Rd& r, int s) {                  // s in 1..15, T.81 F.2.2.1
  const int v = (int)(r.acc >> (64 - s));
  rd_take(r, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// Subsequence `sub` decoded from the packed state `entry`, to the first symbol boundary at or behind its last byte.
// Write = false (speculate, synchronise): nothing but the record.  Write = true: from the true entry state, `blk` its
// first block; non-zero AC coefficients and DC differences go to coef, the true chain's errors to Out::err.
template <bool Write>
VFML_JSYNC_HD Out decode_sub(const Ctx& c, const Tabs& t, int64_t sub, uint32_t entry, int64_t blk, int16_t* coef) {
  Out o;
  o.nblk = 0, o.mark = -1, o.err = 0;
  const int64_t start = sub * c.S;
  const int64_t lim = start + c.S < (int64_t)c.n ? start + c.S : (int64_t)c.n;
  const int64_t lim_bits = lim * 8;
  bool poison = entry == kPoison;
  int b = poison ? 0 : (int)((entry >> 8) & 7u), k = poison ? 0 : (int)((entry >> 11) & 63u);
  if (b >= c.nb) b = 0;
  const int64_t pos0 = start * 8 + (poison ? 0 : (int64_t)(entry & 255u));
  uint32_t iv = interval_of(c, (uint32_t)(pos0 >> 3));
  uint32_t end = interval_end(c, iv, 0u);
  int64_t iend = interval_block0(c, iv + 1);
  Rd r;
  rd_start(r, c, pos0, end);
  const int steps = 9 * c.S + 31;
  for (int it = 0; it < steps; ++it) {
    rd_fill(r, c);
    // the last subsequence's write goes on behind the scan's end, over zeros, as the serial decoder does: a scan that
    // ends before its blocks do is an error of the true chain
    if (r.pos >= lim_bits && !(Write && lim == (int64_t)c.n)) break;
    const bool marker_here = iv < c.nmark && (int64_t)end < lim;
    bool jump = false;
    if (poison) {
      if (!marker_here) break;
      jump = true;
    } else if (Write) {
      if (blk >= iend) {                         // the interval's blocks are done: what is left of it is not decoded
        if (!marker_here) break;
        jump = true;
      } else if (r.pos > (int64_t)end * 8) {
        o.err |= kErrData, poison = true;
        continue;
      }
    } else if (iv < c.nmark && r.pos >= (int64_t)end * 8) {
      jump = true;
    }
    if (jump) {                                  // a restart marker: a known state
      const uint32_t from = end + 2u;
      ++iv;
      end = interval_end(c, iv, from < c.n ? from : c.n);
      iend = interval_block0(c, iv + 1);
      blk = interval_block0(c, iv);
      b = 0, k = 0, poison = false;
      o.nblk = 0, o.mark = (int32_t)iv;
      rd_start(r, c, (int64_t)from * 8, end);
      continue;
    }
    const int comp = b < c.ny ? 0 : b - c.ny + 1;
    bool done = false;
    if (k == 0) {
      const int sym = rd_symbol(r, t, t.dc_t[comp]);
      if (sym < 0) {
        if (Write) o.err |= kErrCode;
        poison = true;
        continue;
      }
      const int s = sym & 15;
      const int diff = s ? rd_extend(r, s) : 0;
      if (Write) coef[blk * 64] = (int16_t)diff;
      k = 1;
    } else {
      const int sym = rd_symbol(r, t, t.ac_t[comp]);
      if (sym < 0) {
        if (Write) o.err |= kErrCode;
        poison = true;
        continue;
      }
      const int run = sym >> 4, s = sym & 15;
      if (s == 0) {
        if (run != 15) {
          done = true;                           // EOB
        } else if (k + 16 > 64) {
          if (Write) o.err |= kErrIndex;
          poison = true;
          continue;
        } else {
          k += 16;                               // ZRL
        }
      } else {
        k += run;
        if (k > 63) {
          if (Write) o.err |= kErrIndex;
          poison = true;
          continue;
        }
        const int val = rd_extend(r, s);
        if (Write) coef[blk * 64 + t.zigzag[k & 63]] = (int16_t)val;
        ++k;
      }
    }
    if (done || k >= 64) {
      k = 0, b = b + 1 >= c.nb ? 0 : b + 1;
      ++o.nblk, ++blk;
      if (Write && r.pos > (int64_t)end * 8) o.err |= kErrData, poison = true;
    }
  }
  o.exit = poison ? kPoison : pack_state(r.pos - lim_bits, b, k);
  return o;
}

// the first block of the subsequence behind one whose first block is `carry`
VFML_JSYNC_HD int64_t place_next(const Ctx& c, int64_t carry, uint32_t nblk, int32_t mark) {
  const int64_t v = (mark >= 0 ? interval_block0(c, (uint32_t)mark) : carry) + nblk;
  return v < 0x7FFFFFFFll ? v : 0x7FFFFFFFll;
}

}  // namespace vfml_jsync
