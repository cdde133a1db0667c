// The self-synchronising JPEG entropy decoder of vfml/csrc/jpeg_decode_sync.hip on the CPU: the same per-subsequence
// steps (vfml/csrc/jpeg_sync_steps.h), the phases run in series.  A stand-alone program, so that the steps can run under
// AddressSanitizer / UBSan without a GPU and without Python in the process (tests/test_jpeg_selfsync_cpu.py):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I video-flow-ml_amd/vfml/csrc tools/jpeg_sync_host.cpp -o jpeg_sync_host
//   jpeg_sync_host case.bin [case.bin ...]
//
// A case file is little-endian int32 h, w, restart interval, subsequence bytes | sampling << 16 (0: 4:2:0, 1: 4:2:2,
// 2: 4:4:4, 3: grey, as VFML_JPEG_* of include/vfml.h), scan bytes, then the 392 int32 of
// storage.jpeg_parse.decode_tables, then the scan.  Per case it prints "status <bits>", "subsequences <n>" and one line
// of 64 coefficients (natural order, DC values summed) per block.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_sync_steps.h"

namespace js = vfml_jsync;

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "jpeg_sync_host: cannot open %s\n", path);
    return 2;
  }
  int32_t head[5];
  std::vector<int32_t> tables(js::kTableInts);
  if (std::fread(head, 4, 5, f) != 5 || std::fread(tables.data(), 4, tables.size(), f) != tables.size()) {
    std::fprintf(stderr, "jpeg_sync_host: %s is too short\n", path);
    std::fclose(f);
    return 2;
  }
  const int h = head[0], w = head[1], dri = head[2], S = head[3] & 0xFFFF, samp = (int)((uint32_t)head[3] >> 16);
  const int64_t n = head[4];
  if (samp > 3 || h < 1 || w < 1 || h > 65535 || w > 65535 || dri < 0 || n < 0 || S < 16 || S > 1024 || (S & (S - 1))) {
    std::fprintf(stderr, "jpeg_sync_host: %s: bad header\n", path);
    std::fclose(f);
    return 2;
  }
  std::vector<uint8_t> scan((size_t)n);
  if (n && std::fread(scan.data(), 1, (size_t)n, f) != (size_t)n) {
    std::fprintf(stderr, "jpeg_sync_host: %s: scan shorter than its header says\n", path);
    std::fclose(f);
    return 2;
  }
  std::fclose(f);

  // the MCU: 16x16 / 16x8 / 8x8 / 8x8 pixels, nb blocks of which the first ny are luma
  const int mw = samp <= 1 ? 16 : 8, mh = samp == 0 ? 16 : 8;
  const int nb = samp == 0 ? 6 : samp == 1 ? 4 : samp == 2 ? 3 : 1, ny = nb == 1 ? 1 : nb - 2;
  const int nmcu = ((h + mh - 1) / mh) * ((w + mw - 1) / mw);
  const int ri = dri > 0 ? dri : nmcu;
  const int nint = (nmcu + ri - 1) / ri;
  int status = 0;
  // markers: count and sequence, as the count / place kernels check them
  std::vector<uint32_t> mpos;
  uint32_t rank = 0;
  for (int64_t p = 0; p + 1 < n; ++p)
    if (scan[(size_t)p] == 0xFF && (scan[(size_t)p + 1] & 0xF8) == 0xD0) {
      if (rank + 1 < (uint32_t)nint) mpos.push_back((uint32_t)p);
      if ((uint32_t)(scan[(size_t)p + 1] & 7) != (rank & 7u)) status |= js::kErrSequence;
      ++rank;
    }
  if (rank + 1 != (uint32_t)nint) status |= js::kErrCount;

  std::vector<int16_t> coef((size_t)nmcu * nb * 64, 0);
  const int64_t N = n > 0 ? (n + S - 1) / S : 1;
  if (status == 0) {
    js::Tabs* tabs = new js::Tabs;
    js::tabs_fill(*tabs, tables.data(), kZigzag, 0, 1);
    js::Ctx c;
    c.scan = scan.data(), c.n = (uint32_t)n, c.mpos = mpos.data(), c.nmark = (uint32_t)mpos.size();
    c.ri = ri, c.nmcu = nmcu, c.S = S, c.nb = nb, c.ny = ny;
    std::vector<js::Rec> rec((size_t)N);
    // speculate
    for (int64_t i = 0; i < N; ++i) {
      const js::Out o = js::decode_sub<false>(c, *tabs, i, 0u, 0, nullptr);
      rec[(size_t)i] = js::Rec{0u, o.exit, o.nblk, o.mark};
    }
    // synchronise: sweeps in order until nothing changes, at most as many as there are subsequences
    for (int64_t round = 0; round < N; ++round) {
      bool changed = false;
      for (int64_t i = 1; i < N; ++i)
        if (rec[(size_t)i - 1].exit != rec[(size_t)i].entry) {
          const uint32_t e = rec[(size_t)i - 1].exit;
          const js::Out o = js::decode_sub<false>(c, *tabs, i, e, 0, nullptr);
          rec[(size_t)i] = js::Rec{e, o.exit, o.nblk, o.mark};
          changed = true;
        }
      if (!changed) break;
    }
    // place and write
    int64_t carry = 0;
    for (int64_t i = 0; i < N; ++i) {
      const js::Out o = js::decode_sub<true>(c, *tabs, i, rec[(size_t)i].entry, carry, coef.data());
      status |= o.err;
      carry = js::place_next(c, carry, rec[(size_t)i].nblk, rec[(size_t)i].mark);
    }
    // DC: sums of the differences per component, restarted at every interval, the low 16 bits kept
    for (int m0 = 0; m0 < nmcu; m0 += ri) {
      int32_t pred[3] = {0, 0, 0};
      for (int m = m0; m < m0 + ri && m < nmcu; ++m)
        for (int b = 0; b < nb; ++b) {
          int16_t& dc = coef[((size_t)m * nb + b) * 64];
          int32_t& p = pred[b < ny ? 0 : b - ny + 1];
          p = (int32_t)((uint32_t)p + (uint32_t)(int32_t)dc);
          dc = (int16_t)(uint16_t)((uint32_t)p & 0xFFFFu);
        }
    }
    delete tabs;
  }
  std::printf("case %s\nstatus %d\nsubsequences %lld\n", path, status, (long long)N);
  for (size_t blk = 0; blk < (size_t)nmcu * nb; ++blk) {
    for (int k = 0; k < 64; ++k) std::printf(k ? " %d" : "%d", (int)coef[blk * 64 + k]);
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: jpeg_sync_host case.bin [case.bin ...]\n");
    return 2;
  }
  for (int i = 1; i < argc; ++i) {
    const int rc = run(argv[i]);
    if (rc) return rc;
  }
  return 0;
}
