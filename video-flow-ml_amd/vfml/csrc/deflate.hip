// Deflate and inflate of the flow cache's .npz members.  Literals-only Huffman in independent
// chunks: a workgroup codes one chunk (histogram, code construction by the shared rule of deflate_code.h, bit positions
// from a prefix sum of code lengths, output assembled in LDS dwords), the chunks are compacted by a prefix sum of their
// byte lengths; a wave decodes one chunk.  The CRC-32 is taken per lane, folded per chunk and per member with
// multiplications by x^(8 len) mod P.  All integer, everything on the caller's stream.
#include "deflate_code.h"
#include "vfml_common.h"

namespace vd = vfml_deflate;

namespace {

constexpr int kEncThreads = 256;
constexpr int kMaxChunks = 16000;        // what a zip extra field (16-bit length) can index, rounded down
constexpr int kSlotPad = 16;

__constant__ uint32_t c_pow8[32] = VFML_DEFLATE_POW8;
__constant__ uint8_t c_cl_order[19] = VFML_DEFLATE_CL_ORDER;

__host__ __device__ inline bool chunk_ok(int c) { return c >= 1024 && c <= 32768 && (c & (c - 1)) == 0; }
inline int64_t chunks_of(int64_t raw_bytes, int c) { return (raw_bytes + c - 1) / c; }
inline int64_t round256(int64_t v) { return (v + 255) / 256 * 256; }

__device__ __forceinline__ uint32_t crc_shift_dev(uint32_t v, uint32_t nbytes) {
  for (int k = 0; nbytes; ++k, nbytes >>= 1)
    if (nbytes & 1u) v = vd::gf_mul(v, c_pow8[k]);
  return v;
}

// exclusive prefix sum over the workgroup's 256 threads (4 waves); wsum: 4 LDS words
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* wsum, uint32_t& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t n = __shfl_up(inc, d, 64);
    if (lane >= d) inc += n;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < kEncThreads / 64; ++i) {
    const uint32_t s = wsum[i];
    base += i < wv ? s : 0u;
    total += s;
  }
  __syncthreads();
  return base + inc - v;
}

// `nbits` (<= 16) bits of `value` at bit `pos` of a zeroed LDS dword buffer of `nwords`
__device__ __forceinline__ void put_bits(uint32_t* out32, uint32_t nwords, uint32_t pos, uint32_t value, uint32_t nbits) {
  const uint32_t w = pos >> 5, sh = pos & 31u;
  if (nbits == 0u) return;
  if (w < nwords) atomicOr(&out32[w], value << sh);
  if (sh + nbits > 32u && w + 1u < nwords) atomicOr(&out32[w + 1], value >> (32u - sh));
}

struct alignas(16) EncTables {
  uint32_t count[260];
  uint32_t w[520];
  uint32_t codetab[260];      // bit-reversed code | length << 16
  uint32_t crc_tab[256];
  uint32_t bl[16], first[16];
  uint32_t cl_count[20], cl_w[40], cl_bl[16], cl_first[16], cl_codetab[20];
  uint32_t wsum[4];
  uint32_t m, data_bits, crc, hclen, head_bits, stored, pad0, pad1;
  uint16_t parent[520], sym_of_rank[260], cl_parent[40], cl_sym[20];
  uint8_t lens[272], cl_lens[32];
};

// LDS offset of byte p of the staged chunk: one dword of padding per 128 bytes, so that threads whose runs lie a multiple
// of 128 bytes apart read different banks
__device__ __forceinline__ uint32_t skew(uint32_t p) { return p + 4u * (p >> 7); }

__host__ __device__ inline uint32_t enc_in_bytes(int c) { return (uint32_t)(c + c / 32 + 32); }
__host__ __device__ inline uint32_t enc_out_bytes(int c) { return (uint32_t)(c + kSlotPad); }
inline size_t enc_lds_bytes(int c) { return sizeof(EncTables) + enc_in_bytes(c) + enc_out_bytes(c); }

// One chunk -> its block(s) in the workspace slot, its byte length and its CRC.
__global__ __launch_bounds__(kEncThreads) void deflate_chunk_kernel(const uint8_t* __restrict__ raw, uint32_t raw_bytes,
                                                                    int C, uint32_t crc_init, uint32_t* __restrict__ ws_len,
                                                                    uint32_t* __restrict__ ws_crc,
                                                                    uint32_t* __restrict__ ws_slots) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  EncTables& T = *reinterpret_cast<EncTables*>(smem);
  uint32_t* in32 = reinterpret_cast<uint32_t*>(smem + sizeof(EncTables));
  const uint8_t* in8 = reinterpret_cast<const uint8_t*>(in32);
  uint32_t* out32 = reinterpret_cast<uint32_t*>(smem + sizeof(EncTables) + enc_in_bytes(C));
  uint8_t* out8 = reinterpret_cast<uint8_t*>(out32);
  const uint32_t out_words = enc_out_bytes(C) / 4u;

  const int t = threadIdx.x;
  const uint32_t c = blockIdx.x, n_chunks = gridDim.x;
  const uint32_t begin = c * (uint32_t)C;
  const uint32_t len = min((uint32_t)C, raw_bytes - begin);
  const bool final_chunk = c + 1u == n_chunks;
  const uint8_t* src = raw + begin;
  const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);      // the chunk starts `a` bytes into a dword

  // stage the chunk: aligned dwords, the two edge dwords byte by byte so that nothing outside the chunk is read
  const uint32_t n_in_words = (a + len + 3u) >> 2;
  for (uint32_t j = t; j < n_in_words; j += kEncThreads) {
    const int64_t first_byte = (int64_t)4 * j - a;                           // index in the chunk of the dword's byte 0
    uint32_t v;
    if (first_byte >= 0 && first_byte + 4 <= (int64_t)len) {
      v = *reinterpret_cast<const uint32_t*>(src + first_byte);
    } else {
      v = 0;
      for (int k = 0; k < 4; ++k) {
        const int64_t i = first_byte + k;
        if (i >= 0 && i < (int64_t)len) v |= (uint32_t)src[i] << (8 * k);
      }
    }
    in32[skew(4u * j) >> 2] = v;
  }
  for (int i = t; i < 260; i += kEncThreads) T.count[i] = 0;
  for (uint32_t i = t; i < out_words; i += kEncThreads) out32[i] = 0;
  T.crc_tab[t] = vd::crc_table_entry((uint32_t)t);
  if (t < 16) T.bl[t] = 0;
  if (t < 20) T.cl_count[t] = 0;
  if (t == 0) T.m = 0, T.data_bits = 0, T.crc = 0;
  __syncthreads();

  // histogram and CRC.  Runs are right-aligned: thread t owns bytes [t * per, (t + 1) * per) of the chunk padded IN FRONT
  // to C bytes, so that every thread's run is followed by exactly (255 - t) * per bytes whatever the chunk's length.
  const int per = C / kEncThreads;
  const int log_per = 31 - __clz(per);
  const int lead = C - (int)len;
  const int run0 = max(t * per - lead, 0), run1 = max((t + 1) * per - lead, 0);   // [run0, run1) of the chunk
  uint32_t reg = 0;
  for (int i = run0; i < run1; ++i) {
    const uint32_t b = in8[skew(a + (uint32_t)i)];
    atomicAdd(&T.count[b], 1u);
    reg = T.crc_tab[(reg ^ b) & 255u] ^ (reg >> 8);
  }
  for (int k = 0; k < 8; ++k)
    if (((255 - t) >> k) & 1) reg = vd::gf_mul(reg, c_pow8[log_per + k]);
  if (reg) atomicXor(&T.crc, reg);
  if (t == 0) T.count[256] = 1;
  __syncthreads();

  // literal code lengths: steps 1-5 of deflate_code.h, a thread per symbol, thread 0 for the serial ones
  int rank0 = -1, rank1 = -1;
  if (T.count[t]) {
    rank0 = vd::rank_of(T.count, vd::kLitSyms, t);
    T.sym_of_rank[rank0] = (uint16_t)t;
    T.w[rank0] = T.count[t];
    atomicAdd(&T.m, 1u);
  }
  if (t == 0) {
    rank1 = vd::rank_of(T.count, vd::kLitSyms, 256);
    T.sym_of_rank[rank1] = 256;
    T.w[rank1] = 1;
    atomicAdd(&T.m, 1u);
  }
  __syncthreads();
  const int m = (int)T.m;                       // >= 2: a literal and the end-of-block symbol
  if (t == 0) vd::tree_build(T.w, T.parent, m);
  __syncthreads();
  for (int r = t; r < m; r += kEncThreads) {
    const int d = vd::depth_of(T.parent, m, r);
    atomicAdd(&T.bl[min(d, vd::kLitLimit)], 1u);
  }
  __syncthreads();
  if (t == 0) {
    vd::limit_repair(T.bl, vd::kLitLimit);
    vd::first_codes(T.bl, vd::kLitLimit, T.first);
  }
  __syncthreads();
  T.lens[t] = rank0 >= 0 ? (uint8_t)vd::length_of_rank(T.bl, vd::kLitLimit, rank0) : (uint8_t)0;
  if (t == 0) {
    T.lens[256] = (uint8_t)vd::length_of_rank(T.bl, vd::kLitLimit, rank1);
    T.lens[257] = 1;                            // the two distance codes
    T.lens[258] = 1;
  }
  __syncthreads();
  for (int s = t; s < vd::kLenSyms; s += kEncThreads) {
    const uint32_t l = T.lens[s];
    atomicAdd(&T.cl_count[l], 1u);
    if (s < vd::kLitSyms) {
      T.codetab[s] = l ? (vd::bit_reverse(vd::code_of(T.lens, T.first, s), (int)l) | (l << 16)) : 0u;
      if (l) atomicAdd(&T.data_bits, T.count[s] * l);
    }
  }
  __syncthreads();

  // the code-length code (19 symbols: in series), the header's size, dynamic or stored
  if (t == 0) {
    vd::lengths_serial(T.cl_count, vd::kClSyms, vd::kClLimit, T.cl_w, T.cl_parent, T.cl_sym, T.cl_bl, T.cl_lens);
    vd::first_codes(T.cl_bl, vd::kClLimit, T.cl_first);
    uint32_t hclen = 4, bits = 0;
    for (int i = 0; i < vd::kClSyms; ++i) {
      const uint32_t l = T.cl_lens[i];
      T.cl_codetab[i] = l ? (vd::bit_reverse(vd::code_of(T.cl_lens, T.cl_first, i), (int)l) | (l << 16)) : 0u;
      bits += T.cl_count[i] * l;
      if (T.cl_lens[c_cl_order[i]] && (uint32_t)i + 1u > hclen) hclen = (uint32_t)i + 1u;
    }
    T.hclen = hclen;
    T.head_bits = 17u + 3u * hclen + bits;
    const uint32_t dyn_bytes = (T.head_bits + T.data_bits + 7u) >> 3;
    T.stored = 5u + len <= dyn_bytes ? 1u : 0u;
  }
  __syncthreads();

  uint32_t chunk_len;
  if (T.stored) {
    if (t == 0) {
      out8[0] = final_chunk ? 1 : 0;
      out8[1] = (uint8_t)(len & 255u), out8[2] = (uint8_t)(len >> 8);
      out8[3] = (uint8_t)(~len & 255u), out8[4] = (uint8_t)((~len >> 8) & 255u);
    }
    for (uint32_t i = t; i < len; i += kEncThreads) out8[5u + i] = in8[skew(a + i)];
    chunk_len = 5u + len;
    if (!final_chunk) {
      if (t == 0) out8[chunk_len + 3] = 0xFF, out8[chunk_len + 4] = 0xFF;     // 00 | 00 00 FF FF (the buffer is zeroed)
      chunk_len += 5u;
    }
  } else {
    const uint32_t head_bits = T.head_bits, hclen = T.hclen;
    if (t == 0) {
      put_bits(out32, out_words, 0, (final_chunk ? 1u : 0u) | (2u << 1), 3);
      put_bits(out32, out_words, 3, 0u | (1u << 5), 10);                      // HLIT = 0 (257 codes), HDIST = 1 (2 codes)
      put_bits(out32, out_words, 13, hclen - 4u, 4);
      for (uint32_t i = 0; i < hclen; ++i) put_bits(out32, out_words, 17u + 3u * i, T.cl_lens[c_cl_order[i]], 3);
    }
    // the 259 code lengths, each as its code-length code
    {
      const uint32_t e = T.cl_codetab[T.lens[t]];
      uint32_t total;
      const uint32_t at = block_scan_excl(e >> 16, T.wsum, total);
      put_bits(out32, out_words, 17u + 3u * hclen + at, e & 0xFFFFu, e >> 16);
      if (t == 0) {
        uint32_t pos = 17u + 3u * hclen + total;
        for (int s = 256; s < vd::kLenSyms; ++s) {
          const uint32_t e2 = T.cl_codetab[T.lens[s]];
          put_bits(out32, out_words, pos, e2 & 0xFFFFu, e2 >> 16);
          pos += e2 >> 16;
        }
      }
    }
    // the literals: bit position of a thread's run = prefix sum of code lengths; words assembled in a 32-bit register
    uint32_t mine = 0;
    for (int i = run0; i < run1; ++i) mine += T.codetab[in8[skew(a + (uint32_t)i)]] >> 16;
    uint32_t total;
    uint32_t pos = head_bits + block_scan_excl(mine, T.wsum, total);
    {
      uint32_t w = pos >> 5, nb = pos & 31u, acc = 0;
      for (int i = run0; i < run1; ++i) {
        const uint32_t e = T.codetab[in8[skew(a + (uint32_t)i)]];
        const uint32_t code = e & 0xFFFFu, l = e >> 16;
        acc |= code << nb;
        if (nb + l >= 32u) {
          if (w < out_words) atomicOr(&out32[w], acc);
          ++w;
          acc = nb + l > 32u ? code >> (32u - nb) : 0u;
          nb = nb + l - 32u;
        } else {
          nb += l;
        }
      }
      if (nb && acc && w < out_words) atomicOr(&out32[w], acc);
    }
    const uint32_t eob = T.codetab[256];
    if (t == 0) put_bits(out32, out_words, head_bits + total, eob & 0xFFFFu, eob >> 16);
    const uint32_t bits = head_bits + total + (eob >> 16);
    if (final_chunk) {
      chunk_len = (bits + 7u) >> 3;
    } else {
      chunk_len = ((bits + 3u + 7u) >> 3) + 4u;       // 3 header bits of the empty stored block, padding, 00 00 FF FF
      __syncthreads();
      if (t == 0) out8[chunk_len - 2] = 0xFF, out8[chunk_len - 1] = 0xFF;
    }
  }
  __syncthreads();

  uint32_t* slot = ws_slots + (size_t)c * (enc_out_bytes(C) / 4u);
  for (uint32_t i = t; i < ((chunk_len + 3u) >> 2); i += kEncThreads) slot[i] = out32[i];
  if (t == 0) {
    const uint32_t init = c == 0 ? crc_init : 0u;
    ws_len[c] = chunk_len;
    ws_crc[c] = ~(crc_shift_dev(~init, len) ^ T.crc);
  }
}

// XOR over the chunks of crc_c * x^(8 * bytes after chunk c): the member's CRC (every thread gets it)
__device__ uint32_t combine_crcs(const uint32_t* ws_crc, uint32_t n_chunks, int C, uint32_t raw_bytes, uint32_t* lds_word) {
  if (threadIdx.x == 0) *lds_word = 0;
  __syncthreads();
  uint32_t acc = 0;
  for (uint32_t c = threadIdx.x; c < n_chunks; c += blockDim.x) {
    const uint32_t end = min((c + 1u) * (uint32_t)C, raw_bytes);
    acc ^= crc_shift_dev(ws_crc[c], raw_bytes - end);
  }
  if (acc) atomicXor(lds_word, acc);
  __syncthreads();
  return *lds_word;
}

// offsets = exclusive prefix sum of the chunks' byte lengths; the stream's length; the member's CRC
__global__ __launch_bounds__(kEncThreads) void deflate_layout_kernel(const uint32_t* __restrict__ ws_len,
                                                                     const uint32_t* __restrict__ ws_crc, uint32_t n_chunks,
                                                                     int C, uint32_t raw_bytes, uint32_t* __restrict__ offsets,
                                                                     uint32_t* __restrict__ stream_bytes,
                                                                     uint32_t* __restrict__ crc) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t word;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_chunks; base += kEncThreads) {
    const uint32_t c = base + threadIdx.x;
    const uint32_t v = c < n_chunks ? ws_len[c] : 0u;
    uint32_t total;
    const uint32_t at = block_scan_excl(v, wsum, total);
    if (c < n_chunks) offsets[c] = carry + at;
    carry += total;
  }
  const uint32_t all = combine_crcs(ws_crc, n_chunks, C, raw_bytes, &word);
  if (threadIdx.x == 0) {
    *stream_bytes = carry;
    *crc = all;
  }
}

// chunk c's bytes from its slot to out + offsets[c]; nothing at or past out + capacity
__global__ __launch_bounds__(kEncThreads) void deflate_compact_kernel(const uint32_t* __restrict__ ws_len,
                                                                      const uint32_t* __restrict__ ws_slots, int C,
                                                                      const uint32_t* __restrict__ offsets,
                                                                      uint8_t* __restrict__ out, int64_t capacity) {
  const uint32_t c = blockIdx.x;
  const uint32_t* slot = ws_slots + (size_t)c * (enc_out_bytes(C) / 4u);
  const int64_t off = offsets[c];
  int64_t n = ws_len[c];
  if (off >= capacity) return;
  if (off + n > capacity) n = capacity - off;
  uint8_t* dst = out + off;
  // bytes up to the first aligned dword of the destination, aligned dwords funnelled out of two slot words, bytes again
  const uint32_t head = min((uint32_t)n, (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
  const uint32_t body = ((uint32_t)n - head) >> 2;
  const uint8_t* slot8 = reinterpret_cast<const uint8_t*>(slot);
  if (threadIdx.x < head) dst[threadIdx.x] = slot8[threadIdx.x];
  uint32_t* dst32 = reinterpret_cast<uint32_t*>(dst + head);
  const uint32_t sh = 8u * (head & 3u);
  for (uint32_t i = threadIdx.x; i < body; i += kEncThreads) {
    const uint32_t s = head + 4u * i;                 // source byte; (s >> 2) + 1 stays inside the padded slot
    const uint32_t lo = slot[s >> 2], hi = slot[(s >> 2) + 1u];
    dst32[i] = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
  }
  const uint32_t tail0 = head + 4u * body;
  if (tail0 + threadIdx.x < (uint32_t)n) dst[tail0 + threadIdx.x] = slot8[tail0 + threadIdx.x];
}

// ---- inflater -------------------------------------------------------------------------------------------------------
constexpr int kLutBits = 10;

struct alignas(16) DecTables {
  uint32_t crc_tab[256];
  uint32_t cnt[16], first[16], offs[16];
  uint32_t produced, status, kind, over, src, n, pad0, pad1;
  uint16_t lut[1 << kLutBits];     // symbol | length << 9; 0: no code of <= kLutBits bits
  uint16_t sorted[320];            // symbols ordered by (length, symbol)
  uint8_t lens[320];
};

__host__ __device__ inline uint32_t dec_in_cap(int c) { return (uint32_t)(c + c / 8 + 64); }   // fixed codes: 9/8
inline size_t dec_lds_bytes(int c) { return sizeof(DecTables) + dec_in_cap(c) + 16 + (size_t)c; }

// canonical decoding tables of lens[0..n) by the whole wave; T.over = 1 for an over-subscribed code
__device__ void build_dec(DecTables& T, int n, int lutbits) {
  const int lane = threadIdx.x;
  if (lane < 16) T.cnt[lane] = 0;
  for (int i = lane; i < (1 << lutbits); i += 64) T.lut[i] = 0;
  __syncthreads();
  for (int s = lane; s < n; s += 64)
    if (T.lens[s]) atomicAdd(&T.cnt[T.lens[s] & 15], 1u);
  __syncthreads();
  if (lane == 0) {
    uint32_t code = 0, off = 0;
    int left = 1;
    T.first[0] = 0, T.offs[0] = 0;
    for (int l = 1; l <= 15; ++l) {
      code = (code + (l > 1 ? T.cnt[l - 1] : 0u)) << 1;
      T.first[l] = code;
      T.offs[l] = off;
      off += T.cnt[l];
      left = (left << 1) - (int)T.cnt[l];
      if (left < 0) left = -(1 << 20);              // over-subscribed, and stays so
    }
    T.over = left < 0 ? 1u : 0u;
  }
  __syncthreads();
  if (T.over) return;
  for (int s = lane; s < n; s += 64) {
    const int l = T.lens[s] & 15;
    if (!l) continue;
    uint32_t k = 0;
    for (int j = 0; j < s; ++j) k += (T.lens[j] & 15) == l ? 1u : 0u;
    T.sorted[T.offs[l] + k] = (uint16_t)s;          // offs[l] + k < n <= 320
    if (l <= lutbits) {
      const uint32_t rev = vd::bit_reverse(T.first[l] + k, l);
      for (uint32_t i = rev; i < (1u << lutbits); i += 1u << l) T.lut[i] = (uint16_t)(s | (l << 9));
    }
  }
  __syncthreads();
}

struct Bits {
  uint32_t buf;
  int cnt;
  uint32_t pos;       // next byte of the staged chunk
};

__device__ __forceinline__ void refill(Bits& b, const uint8_t* in8, uint32_t nbytes) {
  while (b.cnt <= 24) {
    const uint32_t v = b.pos < nbytes ? in8[b.pos] : 0u;
    b.buf |= v << b.cnt;
    b.cnt += 8;
    ++b.pos;
  }
}
__device__ __forceinline__ int bits_left(const Bits& b, uint32_t nbytes) { return b.cnt + 8 * ((int)nbytes - (int)b.pos); }
__device__ __forceinline__ uint32_t take(Bits& b, int k) {
  const uint32_t v = b.buf & ((1u << k) - 1u);
  b.buf >>= k;
  b.cnt -= k;
  return v;
}

// one symbol; -1: the next bits are no code of this table
__device__ __forceinline__ int decode_sym(Bits& b, const DecTables& T, int lutbits) {
  const uint32_t e = T.lut[b.buf & ((1u << lutbits) - 1u)];
  if (e) {
    take(b, (int)(e >> 9));
    return (int)(e & 511u);
  }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)((b.buf >> (l - 1)) & 1u);
    const int count = (int)T.cnt[l];
    if (code - count < first) {
      take(b, l);
      return (int)T.sorted[min(index + (code - first), 319)];
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

// A wave per chunk: lane 0 walks the bits, the wave builds the tables, copies and takes the CRC.
__global__ __launch_bounds__(64) void inflate_chunk_kernel(const uint8_t* __restrict__ data, uint32_t data_bytes,
                                                           const uint32_t* __restrict__ offsets, uint32_t n_chunks, int C,
                                                           uint32_t raw_bytes, uint32_t crc_init, uint32_t* __restrict__ ws_crc,
                                                           uint8_t* __restrict__ raw, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  DecTables& T = *reinterpret_cast<DecTables*>(smem);
  uint8_t* in8 = smem + sizeof(DecTables);
  uint8_t* out8 = smem + sizeof(DecTables) + dec_in_cap(C) + 16;
  const int lane = threadIdx.x;
  const uint32_t c = blockIdx.x;
  const uint32_t want = min((uint32_t)C, raw_bytes - c * (uint32_t)C);
  const uint32_t a = offsets[c];
  const uint32_t b_end = c + 1u < n_chunks ? offsets[c + 1] : data_bytes;
  if (a > b_end || b_end > data_bytes || b_end - a > dec_in_cap(C)) {
    if (lane == 0) {
      atomicOr(status, VFML_INFLATE_ERR_CHUNK);
      ws_crc[c] = 0;
    }
    return;
  }
  const uint32_t nbytes = b_end - a;
  for (uint32_t i = lane; i < nbytes; i += 64) in8[i] = data[a + i];
  for (int i = lane; i < 256; i += 64) T.crc_tab[i] = vd::crc_table_entry((uint32_t)i);
  if (lane == 0) T.produced = 0, T.status = 0;
  __syncthreads();

  Bits bs{0u, 0, 0u};
  for (;;) {
    // block header (lane 0); a stored block is copied by the wave
    if (lane == 0) {
      uint32_t kind = 4;                             // 4: stop
      if (bits_left(bs, nbytes) > 0) {
        refill(bs, in8, nbytes);
        const uint32_t hdr = take(bs, 3);
        kind = ((hdr >> 1) & 3u) | ((hdr & 1u) << 3);            // bit 3: BFINAL
        const uint32_t type = kind & 3u;
        if (bits_left(bs, nbytes) < 0) {
          T.status |= VFML_INFLATE_ERR_BITS, kind = 4;
        } else if (type == 3u) {
          T.status |= VFML_INFLATE_ERR_CODE, kind = 4;
        } else if (type == 0u) {
          take(bs, bs.cnt & 7);
          bs.pos -= (uint32_t)bs.cnt >> 3;           // whole bytes still in the register go back
          bs.buf = 0, bs.cnt = 0;
          if (bs.pos + 4u > nbytes) {
            T.status |= VFML_INFLATE_ERR_BITS, kind = 4;
          } else {
            const uint32_t ln = in8[bs.pos] | ((uint32_t)in8[bs.pos + 1] << 8);
            const uint32_t nl = in8[bs.pos + 2] | ((uint32_t)in8[bs.pos + 3] << 8);
            bs.pos += 4;
            if ((ln ^ nl) != 0xFFFFu) {
              T.status |= VFML_INFLATE_ERR_STORED, kind = 4;
            } else if (bs.pos + ln > nbytes) {
              T.status |= VFML_INFLATE_ERR_BITS, kind = 4;
            } else if (T.produced + ln > want) {
              T.status |= VFML_INFLATE_ERR_LENGTH, kind = 4;
            } else {
              T.src = bs.pos, T.n = ln;
              bs.pos += ln;
            }
          }
        } else if (type == 2u) {
          refill(bs, in8, nbytes);
          const uint32_t hlit = take(bs, 5) + 257u, hdist = take(bs, 5) + 1u, hclen = take(bs, 4) + 4u;
          for (int i = 0; i < 19; ++i) T.lens[i] = 0;
          for (uint32_t i = 0; i < hclen; ++i) {
            refill(bs, in8, nbytes);
            T.lens[c_cl_order[i]] = (uint8_t)take(bs, 3);
          }
          T.src = hlit, T.n = hlit + hdist;
          if (hlit > 286u || hdist > 30u)
            T.status |= VFML_INFLATE_ERR_CODE, kind = 4;
          else if (bits_left(bs, nbytes) < 0)
            T.status |= VFML_INFLATE_ERR_BITS, kind = 4;
        }
      }
      T.kind = kind;
    }
    __syncthreads();
    const uint32_t kind = T.kind, type = kind & 3u;
    if (kind == 4u) break;
    if (type == 0u) {
      const uint32_t src = T.src, n = T.n, at = T.produced;     // at + n <= want <= C, src + n <= nbytes: checked above
      for (uint32_t i = lane; i < n; i += 64) out8[at + i] = in8[src + i];
      __syncthreads();
      if (lane == 0) T.produced = at + n;
    } else {
      int nlit = 288;
      if (type == 2u) {
        build_dec(T, 19, 7);                         // the code-length code
        __syncthreads();
        if (lane == 0) {
          uint32_t st = T.over ? (uint32_t)VFML_INFLATE_ERR_CODE : 0u;
          const uint32_t total = T.n;                // <= 316
          uint32_t got = 0, prev = 0;
          while (!st && got < total) {
            refill(bs, in8, nbytes);
            const int s = decode_sym(bs, T, 7);
            if (s < 0 || s > 18) {
              st = VFML_INFLATE_ERR_CODE;
              break;
            }
            uint32_t rep = 1, val = (uint32_t)s;
            if (s == 16) {
              if (got == 0) {
                st = VFML_INFLATE_ERR_CODE;
                break;
              }
              val = prev, rep = 3u + take(bs, 2);
            } else if (s == 17) {
              val = 0, rep = 3u + take(bs, 3);
            } else if (s == 18) {
              val = 0, rep = 11u + take(bs, 7);
            }
            if (bits_left(bs, nbytes) < 0) {
              st = VFML_INFLATE_ERR_BITS;
              break;
            }
            if (got + rep > total) {
              st = VFML_INFLATE_ERR_CODE;
              break;
            }
            // the code-length code's own lengths sit in T.lens[0..19) and its tables are built: overwrite from 0
            for (uint32_t i = 0; i < rep; ++i) T.lens[got + i] = (uint8_t)val;
            got += rep;
            prev = val;
          }
          if (st) T.status |= st, T.kind = 4;
        }
        __syncthreads();
        if (T.kind == 4u) break;
        nlit = (int)T.src;
      } else {
        for (int s = lane; s < 288; s += 64) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        __syncthreads();
      }
      build_dec(T, nlit, kLutBits);
      __syncthreads();
      if (lane == 0) {
        uint32_t st = T.over ? (uint32_t)VFML_INFLATE_ERR_CODE : 0u;
        uint32_t at = T.produced;
        while (!st) {
          refill(bs, in8, nbytes);
          const int s = decode_sym(bs, T, kLutBits);
          if (bits_left(bs, nbytes) < 0) {
            st = VFML_INFLATE_ERR_BITS;
          } else if (s < 0) {
            st = VFML_INFLATE_ERR_CODE;
          } else if (s == 256) {
            break;
          } else if (s > 256) {
            st = VFML_INFLATE_ERR_MATCH;
          } else if (at >= want) {
            st = VFML_INFLATE_ERR_LENGTH;
          } else {
            out8[at++] = (uint8_t)s;
          }
        }
        T.produced = at;
        if (st) T.status |= st, T.kind = 4;
      }
      __syncthreads();
      if (T.kind == 4u) break;
    }
    if (kind & 8u) break;                            // BFINAL
    __syncthreads();
  }
  __syncthreads();
  if (lane == 0 && T.status == 0u && T.produced != want) T.status = VFML_INFLATE_ERR_LENGTH;
  __syncthreads();
  const uint32_t produced = min(T.produced, want);
  uint8_t* dst = raw + (size_t)c * (uint32_t)C;
  for (uint32_t i = lane; i < produced; i += 64) dst[i] = out8[i];

  // CRC of the chunk, lanes' runs right-aligned as in the encoder
  const int per = C / 64, log_per = 31 - __clz(per);
  const int lead = C - (int)want;
  const int run0 = max(lane * per - lead, 0), run1 = max((lane + 1) * per - lead, 0);
  uint32_t reg = 0;
  if (T.status == 0u)
    for (int i = run0; i < run1; ++i) reg = T.crc_tab[(reg ^ out8[i]) & 255u] ^ (reg >> 8);
  for (int k = 0; k < 6; ++k)
    if (((63 - lane) >> k) & 1) reg = vd::gf_mul(reg, c_pow8[log_per + k]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) reg ^= __shfl_xor(reg, d, 64);
  if (lane == 0) {
    const uint32_t init = c == 0 ? crc_init : 0u;
    ws_crc[c] = ~(crc_shift_dev(~init, want) ^ reg);
    if (T.status) atomicOr(status, (int32_t)T.status);
  }
}

__global__ __launch_bounds__(kEncThreads) void inflate_crc_kernel(const uint32_t* __restrict__ ws_crc, uint32_t n_chunks, int C,
                                                                  uint32_t raw_bytes, uint32_t* __restrict__ crc) {
  __shared__ uint32_t word;
  const uint32_t all = combine_crcs(ws_crc, n_chunks, C, raw_bytes, &word);
  if (threadIdx.x == 0) *crc = all;
}

}  // namespace

extern "C" {

int64_t vfml_deflate_capacity(int64_t raw_bytes, int chunk_bytes) {
  if (!chunk_ok(chunk_bytes) || raw_bytes < 1 || raw_bytes > 0x7FFFFFFF) return 0;
  const int64_t n = chunks_of(raw_bytes, chunk_bytes);
  if (n > kMaxChunks) return 0;
  return raw_bytes + 10 * n;                       // a stored block (5 + len) and the empty stored block (5) per chunk
}

int64_t vfml_deflate_workspace_bytes(int64_t raw_bytes, int chunk_bytes) {
  if (vfml_deflate_capacity(raw_bytes, chunk_bytes) == 0) return 0;
  const int64_t n = chunks_of(raw_bytes, chunk_bytes);
  return 2 * round256(4 * n) + n * (int64_t)enc_out_bytes(chunk_bytes);
}

int64_t vfml_inflate_workspace_bytes(int64_t raw_bytes, int chunk_bytes) {
  if (vfml_deflate_capacity(raw_bytes, chunk_bytes) == 0) return 0;
  return round256(4 * chunks_of(raw_bytes, chunk_bytes));
}

int vfml_deflate_huffman(const unsigned char* raw, int64_t raw_bytes, int chunk_bytes, uint32_t crc_init, void* workspace,
                         unsigned char* out, int64_t capacity, uint32_t* offsets, uint32_t* stream_bytes, uint32_t* crc,
                         void* stream) {
  VFML_REQUIRE(vfml_deflate_capacity(raw_bytes, chunk_bytes) != 0,
               "vfml_deflate_huffman: %lld bytes in chunks of %d: chunk_bytes is a power of two 1024..32768, 1 <= raw_bytes "
               "< 2 GiB, at most %d chunks", (long long)raw_bytes, chunk_bytes, kMaxChunks);
  VFML_REQUIRE(raw && workspace && out && offsets && stream_bytes && crc, "vfml_deflate_huffman: null pointer");
  VFML_REQUIRE(capacity >= 0, "vfml_deflate_huffman: negative capacity");
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "vfml_deflate_huffman: workspace not 256-byte aligned");
  VFML_REQUIRE(((reinterpret_cast<uintptr_t>(offsets) | reinterpret_cast<uintptr_t>(stream_bytes) |
                 reinterpret_cast<uintptr_t>(crc)) & 3u) == 0, "vfml_deflate_huffman: offsets, stream_bytes, crc: 4-byte aligned");
  const uint32_t n = (uint32_t)chunks_of(raw_bytes, chunk_bytes);
  uint32_t* ws_len = static_cast<uint32_t*>(workspace);
  uint32_t* ws_crc = ws_len + round256(4 * (int64_t)n) / 4;
  uint32_t* ws_slots = ws_crc + round256(4 * (int64_t)n) / 4;
  const size_t lds = enc_lds_bytes(chunk_bytes);
  if (int rc = vfml_lds_cap(reinterpret_cast<const void*>(deflate_chunk_kernel), (int)enc_lds_bytes(32768), "vfml_deflate_huffman"))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(deflate_chunk_kernel, dim3(n), dim3(kEncThreads), lds, s, raw, (uint32_t)raw_bytes, chunk_bytes, crc_init,
                     ws_len, ws_crc, ws_slots);
  hipLaunchKernelGGL(deflate_layout_kernel, dim3(1), dim3(kEncThreads), 0, s, ws_len, ws_crc, n, chunk_bytes,
                     (uint32_t)raw_bytes, offsets, stream_bytes, crc);
  hipLaunchKernelGGL(deflate_compact_kernel, dim3(n), dim3(kEncThreads), 0, s, ws_len, ws_slots, chunk_bytes, offsets, out,
                     capacity);
  return vfml_check_launch("vfml_deflate_huffman");
}

int vfml_inflate_chunks(const unsigned char* data, int64_t data_bytes, const uint32_t* offsets, int n_chunks, int chunk_bytes,
                        int64_t raw_bytes, uint32_t crc_init, void* workspace, unsigned char* raw, uint32_t* crc,
                        int32_t* status, void* stream) {
  VFML_REQUIRE(vfml_deflate_capacity(raw_bytes, chunk_bytes) != 0,
               "vfml_inflate_chunks: %lld bytes in chunks of %d: chunk_bytes is a power of two 1024..32768, 1 <= raw_bytes < "
               "2 GiB, at most %d chunks", (long long)raw_bytes, chunk_bytes, kMaxChunks);
  VFML_REQUIRE(n_chunks == chunks_of(raw_bytes, chunk_bytes), "vfml_inflate_chunks: %d chunks for %lld bytes in chunks of %d",
               n_chunks, (long long)raw_bytes, chunk_bytes);
  VFML_REQUIRE(data_bytes >= 0 && data_bytes <= 0x7FFFFFFF, "vfml_inflate_chunks: data_bytes %lld", (long long)data_bytes);
  VFML_REQUIRE(data && offsets && workspace && raw && crc && status, "vfml_inflate_chunks: null pointer");
  VFML_REQUIRE(((reinterpret_cast<uintptr_t>(offsets) | reinterpret_cast<uintptr_t>(crc) | reinterpret_cast<uintptr_t>(status) |
                 reinterpret_cast<uintptr_t>(workspace)) & 3u) == 0,
               "vfml_inflate_chunks: offsets, crc, status, workspace: 4-byte aligned");
  if (int rc = vfml_lds_cap(reinterpret_cast<const void*>(inflate_chunk_kernel), (int)dec_lds_bytes(32768), "vfml_inflate_chunks"))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), s);
  if (e != hipSuccess) {
    vfml_set_error("vfml_inflate_chunks: hipMemsetAsync: %s", hipGetErrorString(e));
    return 2;
  }
  uint32_t* ws_crc = static_cast<uint32_t*>(workspace);
  hipLaunchKernelGGL(inflate_chunk_kernel, dim3((uint32_t)n_chunks), dim3(64), dec_lds_bytes(chunk_bytes), s, data,
                     (uint32_t)data_bytes, offsets, (uint32_t)n_chunks, chunk_bytes, (uint32_t)raw_bytes, crc_init, ws_crc, raw,
                     status);
  hipLaunchKernelGGL(inflate_crc_kernel, dim3(1), dim3(kEncThreads), 0, s, ws_crc, (uint32_t)n_chunks, chunk_bytes,
                     (uint32_t)raw_bytes, crc);
  return vfml_check_launch("vfml_inflate_chunks");
}

}  // extern "C"
