// The code-construction rule of vfml/csrc/deflate_code.h on the CPU: the same steps the encoder kernel of
// vfml/csrc/deflate.hip runs, in series.  A stand-alone program, so that the steps can run under AddressSanitizer /
// UBSan without a GPU and without Python in the process (tests/test_deflate_cpu.py):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I video-flow-ml_amd/vfml/csrc tools/deflate_code_host.cpp -o deflate_code_host
//   deflate_code_host histograms.txt
//
// A line of the file is "<limit> <n> <count 0> ... <count n-1>".  Per line it prints "lens <len 0> ... <len n-1>" and
// "codes <bit-reversed code 0> ...", the lines tests/deflate_oracle.py prints for the same histogram; then "pow8 ok"
// once the header's table of x^(8 * 2^k) equals its own arithmetic, and "crc <hex>" of the check string "123456789"
// taken in three pieces that are folded with crc_shift.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deflate_code.h"

namespace vd = vfml_deflate;

static uint32_t crc_piece(const unsigned char* p, size_t n, uint32_t init) {
  uint32_t c = ~init;
  for (size_t i = 0; i < n; ++i) c = vd::crc_table_entry((c ^ p[i]) & 255u) ^ (c >> 8);
  return ~c;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: deflate_code_host histograms.txt\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "deflate_code_host: cannot open %s\n", argv[1]);
    return 2;
  }
  int limit, n;
  while (std::fscanf(f, "%d %d", &limit, &n) == 2) {
    if (limit < 1 || limit > vd::kMaxLimit || n < 1 || n > 320) {
      std::fprintf(stderr, "deflate_code_host: bad line header %d %d\n", limit, n);
      std::fclose(f);
      return 2;
    }
    // exact sizes, so that an index past what a step may touch is an AddressSanitizer report
    std::vector<uint32_t> count((size_t)n), w((size_t)2 * n), bl((size_t)limit + 1), first((size_t)limit + 1);
    std::vector<uint16_t> parent((size_t)2 * n), sym((size_t)n);
    std::vector<uint8_t> lens((size_t)n);
    for (int i = 0; i < n; ++i)
      if (std::fscanf(f, "%u", &count[(size_t)i]) != 1) {
        std::fprintf(stderr, "deflate_code_host: short line\n");
        std::fclose(f);
        return 2;
      }
    vd::lengths_serial(count.data(), n, limit, w.data(), parent.data(), sym.data(), bl.data(), lens.data());
    vd::first_codes(bl.data(), limit, first.data());
    std::printf("lens");
    for (int i = 0; i < n; ++i) std::printf(" %d", (int)lens[(size_t)i]);
    std::printf("\ncodes");
    for (int i = 0; i < n; ++i)
      std::printf(" %u", lens[(size_t)i] ? vd::bit_reverse(vd::code_of(lens.data(), first.data(), i), lens[(size_t)i]) : 0u);
    std::printf("\n");
  }
  std::fclose(f);

  const uint32_t table[32] = VFML_DEFLATE_POW8;
  for (int k = 0; k < 32; ++k)
    if (table[k] != vd::pow8_entry(k)) {
      std::printf("pow8 entry %d differs\n", k);
      return 1;
    }
  std::printf("pow8 ok\n");
  const unsigned char* s = reinterpret_cast<const unsigned char*>("123456789");
  const uint32_t a = crc_piece(s, 2, 0), b = crc_piece(s + 2, 4, 0), c = crc_piece(s + 6, 3, 0);
  std::printf("crc %08x\n", vd::crc_shift(a, 7, table) ^ vd::crc_shift(b, 3, table) ^ c);
  return 0;
}
