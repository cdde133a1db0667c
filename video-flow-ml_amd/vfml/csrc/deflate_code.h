// The code-construction rule of the flow cache's deflate streams, written once: the encoder kernel
// (deflate.hip) runs these steps with a thread per element and a lane for the serial ones, tools/deflate_code_host.cpp
// runs them in loops on the CPU (under AddressSanitizer / UBSan, without a GPU), and tests/deflate_oracle.py states the
// same rule in Python.  Everything is integer; no step keeps an array of its own - the caller owns the storage (LDS in
// the kernel).
//
// The rule, for a histogram count[0..n) and a length limit L (15 for literals + end-of-block, 7 for the code-length code):
//   1. the used symbols (count > 0) are ordered by (count, symbol) ascending: rank_of;
//   2. a Huffman tree is built over them with two queues - the ordered leaves and the internal nodes in the order they
//      were made - taking the lighter head each time, THE LEAF ON A TIE: tree_build;
//   3. a leaf's depth (depth_of), clamped to L, is counted into bl_count[1..L]; a single used symbol gets length 1;
//   4. while the Kraft sum exceeds 1 (only after clamping): one code leaves length L, and the longest code shorter than L
//      is replaced by two codes one bit longer: limit_repair;
//   5. lengths are handed out by rank: the rarest symbols get the longest codes: length_of_rank;
//   6. codes are canonical (RFC 1951 3.2.2): first_codes, code_of; sent least-significant bit first, hence bit_reverse.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VFML_DEFLATE_HD __host__ __device__ __forceinline__
#else
#define VFML_DEFLATE_HD inline
#endif

namespace vfml_deflate {

constexpr int kLitSyms = 257;     // literals 0..255 and end-of-block; no length symbol is ever sent (HLIT = 0)
constexpr int kLenSyms = 259;     // + the two distance codes of length 1 that zlib writes for a block without matches
constexpr int kClSyms = 19;
constexpr int kLitLimit = 15;
constexpr int kClLimit = 7;
constexpr int kMaxLimit = 15;

// order in which the code-length code's own lengths are sent (RFC 1951 3.2.7)
#define VFML_DEFLATE_CL_ORDER {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15}

// step 1: position of used symbol s among the used symbols ordered by (count, symbol)
VFML_DEFLATE_HD int rank_of(const uint32_t* count, int n, int s) {
  const uint32_t c = count[s];
  int r = 0;
  for (int j = 0; j < n; ++j) {
    const uint32_t cj = count[j];
    r += (cj != 0u && (cj < c || (cj == c && j < s))) ? 1 : 0;
  }
  return r;
}

// step 2: w[0..m) = the leaves' counts in rank order; nodes m..2m-2 are made here (w[] receives their weights, 2m-1
// entries in all), parent[x] of every node but the root 2m-2.  m >= 2.
VFML_DEFLATE_HD void tree_build(uint32_t* w, uint16_t* parent, int m) {
  int leaf = 0, inode = m;
  for (int next = m; next < 2 * m - 1; ++next) {
    int pick[2];
    for (int k = 0; k < 2; ++k) {
      if (leaf < m && (inode >= next || w[leaf] <= w[inode]))
        pick[k] = leaf++;
      else
        pick[k] = inode++;
    }
    w[next] = w[pick[0]] + w[pick[1]];
    parent[pick[0]] = (uint16_t)next;
    parent[pick[1]] = (uint16_t)next;
  }
}

// step 3: edges from leaf to the root 2m-2
VFML_DEFLATE_HD int depth_of(const uint16_t* parent, int m, int leaf) {
  int d = 0;
  for (int x = leaf; x != 2 * m - 2; x = parent[x]) ++d;
  return d;
}

// step 4: bl_count[1..limit] after clamping -> a complete code (Kraft sum 1) with the same number of symbols
VFML_DEFLATE_HD void limit_repair(uint32_t* bl_count, int limit) {
  uint32_t total = 0;
  for (int i = 1; i <= limit; ++i) total += bl_count[i] << (limit - i);
  while (total > (1u << limit)) {
    bl_count[limit]--;
    for (int i = limit - 1; i > 0; --i)
      if (bl_count[i]) {
        bl_count[i]--;
        bl_count[i + 1] += 2;
        break;
      }
    total--;
  }
}

// step 5: the code length of the used symbol of rank r (rank 0 = rarest = longest)
VFML_DEFLATE_HD int length_of_rank(const uint32_t* bl_count, int limit, int r) {
  uint32_t acc = 0;
  for (int len = limit; len >= 1; --len) {
    acc += bl_count[len];
    if ((uint32_t)r < acc) return len;
  }
  return 0;
}

// steps 1-5 in series: lens[0..n) of count[0..n).  w: 2n entries, parent: 2n, sym: n, bl: limit + 1.
VFML_DEFLATE_HD void lengths_serial(const uint32_t* count, int n, int limit, uint32_t* w, uint16_t* parent, uint16_t* sym,
                                    uint32_t* bl, uint8_t* lens) {
  int m = 0;
  for (int s = 0; s < n; ++s) {
    lens[s] = 0;
    if (count[s]) {
      const int r = rank_of(count, n, s);
      sym[r] = (uint16_t)s;
      w[r] = count[s];
      ++m;
    }
  }
  for (int i = 0; i <= limit; ++i) bl[i] = 0;
  if (m == 0) return;
  if (m == 1) {
    bl[1] = 1;
  } else {
    tree_build(w, parent, m);
    for (int r = 0; r < m; ++r) {
      const int d = depth_of(parent, m, r);
      bl[d < limit ? d : limit]++;
    }
    limit_repair(bl, limit);
  }
  for (int r = 0; r < m; ++r) lens[sym[r]] = (uint8_t)length_of_rank(bl, limit, r);
}

// step 6: first[len] = the first canonical code of that length (first[0..limit])
VFML_DEFLATE_HD void first_codes(const uint32_t* bl_count, int limit, uint32_t* first) {
  uint32_t code = 0;
  first[0] = 0;
  for (int bits = 1; bits <= limit; ++bits) {
    code = (code + (bits > 1 ? bl_count[bits - 1] : 0u)) << 1;
    first[bits] = code;
  }
}

VFML_DEFLATE_HD uint32_t code_of(const uint8_t* lens, const uint32_t* first, int s) {
  const int len = lens[s];
  uint32_t k = 0;
  for (int j = 0; j < s; ++j) k += lens[j] == len ? 1u : 0u;
  return first[len] + k;
}

VFML_DEFLATE_HD uint32_t bit_reverse(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// ---- CRC-32 (the zip / zlib polynomial, reflected: bit 31 of a word is x^0) -----------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;

VFML_DEFLATE_HD uint32_t crc_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}

// a(x) * b(x) mod P
VFML_DEFLATE_HD uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= (a & (0x80000000u >> i)) ? b : 0u;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

// x^(8 * 2^k) mod P, k = 0..31
VFML_DEFLATE_HD uint32_t pow8_entry(int k) {
  uint32_t p = 0x00800000u;                  // x^8
  for (int i = 0; i < k; ++i) p = gf_mul(p, p);
  return p;
}

// pow8_entry(0..31) as literals, for a table in the GPU's constant memory (tools/deflate_code_host.cpp compares the two)
#define VFML_DEFLATE_POW8                                                                                              \
  {0x00800000u, 0x00008000u, 0xEDB88320u, 0xB1E6B092u, 0xA06A2517u, 0xED627DAEu, 0x88D14467u, 0xD7BBFE6Au, 0xEC447F11u, \
   0x8E7EA170u, 0x6427800Eu, 0x4D47BAE0u, 0x09FE548Fu, 0x83852D0Fu, 0x30362F1Au, 0x7B5A9CC3u, 0x31FEC169u, 0x9FEC022Au, \
   0x6C8DEDC4u, 0x15D6874Du, 0x5FDE7A4Eu, 0xBAD90E37u, 0x2E4E5EEFu, 0x4EABA214u, 0xA8A472C0u, 0x429A969Eu, 0x148D302Au, \
   0xC40BA6D0u, 0xC4E22C3Cu, 0x40000000u, 0x20000000u, 0x08000000u}

// v * x^(8 * nbytes) mod P with pow8[k] = pow8_entry(k): what `nbytes` zero bytes do to a CRC register, and the factor
// of zlib's crc32_combine
VFML_DEFLATE_HD uint32_t crc_shift(uint32_t v, uint32_t nbytes, const uint32_t* pow8) {
  for (int k = 0; nbytes; ++k, nbytes >>= 1)
    if (nbytes & 1u) v = gf_mul(v, pow8[k]);
  return v;
}

}  // namespace vfml_deflate
