// vfml_jpeg_encode_rgb: the baseline JPEG of the output video's MJPG frames - 8-bit, YCbCr 4:2:0,
// the Annex K tables unoptimised, one MCU row per restart interval.  Integer arithmetic only; tests/jpeg_oracle.py is the
// same definition in numpy and the stream equals its stream byte for byte.  The constant tables (zigzag, DCT matrix,
// Huffman codes) are jpeg_tables.inc, printed from storage/jpeg_tables.py, the module that writes the file header.
// vfml_jpeg_encode_rgb_sampled is the same encoder for 4:2:0, 4:2:2 and 4:4:4 (tests/jpeg_encode_sampling_oracle.py): the
// sampling is a template parameter of the two kernels that know the MCU, and their 4:2:0 instantiation is the code of
// vfml_jpeg_encode_rgb, which forwards to it.
//
// Five launches on one stream, no host pass over the entropy data and no synchronisation:
//   transform   one wave per region of 16 x 16 pixels, 4 per lane - one 4:2:0 MCU, two 4:2:2 MCUs one above the other or
//               four 4:4:4 MCUs: colour conversion, the chroma sample (4:2:0: 2x2 mean across lanes; 4:2:2: the pair's mean
//               in the lane; 4:4:4: the sample), both DCT passes through LDS, quantisation; int16 coefficients in zigzag
//               order, the blocks of an MCU in scan order, MCUs in raster order.
//   entropy     one wave per 8 x 8 block, one lane per coefficient: the ballot of "non-zero" gives a lane its zero run and
//               the end of block, a wave prefix sum its bit offset; the lanes OR their codes into the block's bit string
//               in LDS (at most 1660 bits) and the used words and the bit length go to the workspace.
//   interval    one workgroup per MCU row: scans the blocks' bit lengths, then every thread assembles one 32-bit word of
//               the interval from the blocks that overlap it (a binary search in the scanned offsets), pads the tail with
//               1-bits, counts its FF bytes, and a workgroup scan places the stuffed bytes in the row's staging area;
//               RSTm follows every interval but the last.
//   offsets     scans the intervals' byte lengths; the total goes to the caller's cell.
//   compact     copies the staged rows into one contiguous scan, never past the caller's capacity.
// Every workspace region is sized for the worst case (a block: 1660 bits, 416 bytes after stuffing), so no kernel can
// write outside it whatever the picture holds.
#include "vfml_common.h"

namespace {

#include "jpeg_tables.inc"

constexpr int kBlockWords = 52;           // 32-bit words of a block's bit string: 1660 bits at most
constexpr int kBlockBytesMax = 416;       // of one block in the scan: 1660 bits, every byte stuffed
constexpr int kIntervalThreads = 1024;

struct JpegArgs {
  const unsigned char* rgb;
  int h, w;
  int64_t stride;
  const unsigned char* qt;                // [2][64] natural order
  int rows, cols;                         // MCU rows, MCUs per row
  int bpm;                                // blocks per MCU
  int rrows, rcols;                       // the transform's 16 x 16 regions
  short* coef;                            // [blocks][64] zigzag
  unsigned* bits;                         // [blocks][kBlockWords]
  unsigned* blen;                         // [blocks] bit length
  unsigned* boff;                         // [blocks] bit offset in its interval
  unsigned char* stage;                   // [rows][row_cap]
  int64_t row_cap;
  unsigned* ilen;                         // [rows] bytes of the interval, RSTm included
  unsigned* ioff;                         // [rows] byte offset in the scan
  unsigned char* scan;
  int64_t cap;
  unsigned* total;
};

__host__ __device__ inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// ---- transform ---------------------------------------------------------------------------------------------------
// The MCU of a sampling (VFML_JPEG_420 / 422 / 444) and the 16 x 16 pixel region one wave transforms.
template <int S>
struct Mcu {
  static constexpr int kLumaV = S == 0 ? 2 : 1, kLumaH = S == 2 ? 1 : 2;  // luma blocks down and across an MCU
  static constexpr int kLuma = kLumaV * kLumaH;
  static constexpr int kBlocks = kLuma + 2;                                 // Y .. Cb Cr
  static constexpr int kRegionV = 2 / kLumaV, kRegionH = 2 / kLumaH;        // MCUs down and across a region
  static constexpr int kRegionBlocks = kRegionV * kRegionH * kBlocks;       // 6, 8, 12
};

template <int S>
__global__ __launch_bounds__(256) void jpeg_transform_kernel(const JpegArgs a) {
  using M = Mcu<S>;
  constexpr int NB = M::kRegionBlocks;
  __shared__ int xs[4][NB][64];
  __shared__ int ts[4][NB][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nmcu = a.rrows * a.rcols;
  int mcu = blockIdx.x * 4 + wave;
  const bool valid = mcu < nmcu;
  if (!valid) mcu = nmcu - 1;
  const int my = mcu / a.rcols, mx = mcu - my * a.rcols;
  // lane -> row r of the region, columns 4q .. 4q+3
  const int r = lane >> 2, q = lane & 3;
  int py = my * 16 + r;
  py = py < a.h ? py : a.h - 1;
  const unsigned char* row = a.rgb + (int64_t)py * a.stride;
  int cbs[2], crs[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int px = mx * 16 + 4 * q + j;
    px = px < a.w ? px : a.w - 1;
    const int R = row[3 * px], G = row[3 * px + 1], B = row[3 * px + 2];
    const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    const int Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    const int Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    const int c = 4 * q + j;
    if constexpr (S == 0) {
      xs[wave][(r >> 3) * 2 + (c >> 3)][(r & 7) * 8 + (c & 7)] = Y - 128;
    } else if constexpr (S == 1) {        // MCU r >> 3 of the region: Y0 Y1 Cb Cr
      xs[wave][(r >> 3) * 4 + (c >> 3)][(r & 7) * 8 + (c & 7)] = Y - 128;
    } else {                              // MCU (r >> 3, c >> 3) of the region: Y Cb Cr
      const int at = (r & 7) * 8 + (c & 7), b0 = ((r >> 3) * 2 + (c >> 3)) * 3;
      xs[wave][b0][at] = Y - 128;
      xs[wave][b0 + 1][at] = Cb - 128;
      xs[wave][b0 + 2][at] = Cr - 128;
    }
    if constexpr (S != 2) {
      if (j & 1) {
        cbs[j >> 1] += Cb;
        crs[j >> 1] += Cr;
      } else {
        cbs[j >> 1] = Cb;
        crs[j >> 1] = Cr;
      }
    }
  }
  if constexpr (S == 0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {         // the other row of the 2x2 cell is four lanes away
      const int cb = cbs[p] + __shfl_xor(cbs[p], 4), cr = crs[p] + __shfl_xor(crs[p], 4);
      if (!(r & 1)) {
        const int at = (r >> 1) * 8 + 2 * q + p;
        xs[wave][4][at] = ((cb + 2) >> 2) - 128;
        xs[wave][5][at] = ((cr + 2) >> 2) - 128;
      }
    }
  } else if constexpr (S == 1) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {         // the horizontal pair is the lane's own
      const int at = (r & 7) * 8 + 2 * q + p;
      xs[wave][(r >> 3) * 4 + 2][at] = ((cbs[p] + 1) >> 1) - 128;
      xs[wave][(r >> 3) * 4 + 3][at] = ((crs[p] + 1) >> 1) - 128;
    }
  }
  __syncthreads();
  // pass 1: T = (C X + 1024) >> 11, lane = (k, n)
  {
    const int k = lane >> 3, n = lane & 7;
    int ck[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) ck[m] = kJpegDct[k * 8 + m];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      int acc = 1024;
#pragma unroll
      for (int m = 0; m < 8; ++m) acc += ck[m] * xs[wave][b][m * 8 + n];
      ts[wave][b][lane] = acc >> 11;
    }
  }
  __syncthreads();
  // pass 2: Y = (T C^T + 16384) >> 15 and quantisation, lane = zigzag position
  {
    const int nat = kJpegZigzag[lane];
    const int k = nat >> 3, l = nat & 7;
    int cl[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) cl[n] = kJpegDct[l * 8 + n];
    const int q0 = a.qt[nat], q1 = a.qt[64 + nat];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      int acc = 16384;
#pragma unroll
      for (int n = 0; n < 8; ++n) acc += ts[wave][b][k * 8 + n] * cl[n];
      const int y = acc >> 15;
      const int qq = b % M::kBlocks < M::kLuma ? q0 : q1;
      int v = ((y < 0 ? -y : y) + (qq >> 1)) / qq;
      if (lane > 0 && v > 1023) v = 1023;
      if (y < 0) v = -v;
      if constexpr (S == 0) {
        if (valid) a.coef[((int64_t)mcu * 6 + b) * 64 + lane] = (short)v;
      } else {                            // block b of the region -> its MCU, which may lie outside the grid
        constexpr int kPerRow = M::kRegionH;
        const int m = b / M::kBlocks;
        const int gy = my * M::kRegionV + m / kPerRow, gx = mx * kPerRow + m % kPerRow;
        if (valid && gy < a.rows && gx < a.cols)
          a.coef[(((int64_t)gy * a.cols + gx) * M::kBlocks + b % M::kBlocks) * 64 + lane] = (short)v;
      }
    }
  }
}

// ---- entropy -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int bit_size(int v) { return 32 - __clz(v < 0 ? -v : v); }

// `len` bits (1..32) of v, most significant first, at bit `at` of the string
__device__ __forceinline__ void put_bits(unsigned* words, unsigned at, unsigned v, int len) {
  const int wd = at >> 5, sh = at & 31;
  const unsigned long long x = (unsigned long long)v << (64 - len - sh);
  atomicOr(&words[wd], (unsigned)(x >> 32));
  if (sh + len > 32) atomicOr(&words[wd + 1], (unsigned)x);
}

template <int S>
__global__ __launch_bounds__(256) void jpeg_entropy_kernel(const JpegArgs a) {
  constexpr int BPM = Mcu<S>::kBlocks, LUMA = Mcu<S>::kLuma;
  __shared__ unsigned words[4][kBlockWords];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t nblk = (int64_t)a.rows * a.cols * BPM;
  int64_t g = (int64_t)blockIdx.x * 4 + wave;
  const bool valid = g < nblk;
  if (!valid) g = nblk - 1;
  const int64_t mcu = g / BPM;
  const int b = (int)(g - mcu * BPM);
  const int col = (int)(mcu % a.cols);
  const int tc = b < LUMA ? 0 : 1;
  if (lane < kBlockWords) words[wave][lane] = 0;
  int c = a.coef[g * 64 + lane];
  if (lane > 0) c = c < -1023 ? -1023 : (c > 1023 ? 1023 : c);     // (as written by the transform: bounds the bit string)
  const bool nz = lane > 0 && c != 0;
  const unsigned long long mask = __ballot(nz);
  const unsigned zrl = kJpegHuffAC[tc][0xF0];
  const int zrl_len = zrl & 31;
  unsigned piece = 0;                     // the lane's code and value bits
  int plen = 0, nzrl = 0;
  if (lane == 0) {
    int pred = 0;                         // the previous block of the component in this interval
    if (b > 0 && b < LUMA)
      pred = a.coef[(g - 1) * 64];
    else if (col > 0)                     // the last luma block, or the same chroma block, of the MCU in front
      pred = a.coef[(b == 0 ? g - BPM + LUMA - 1 : g - BPM) * 64];
    int d = c - pred;
    d = d < -2047 ? -2047 : (d > 2047 ? 2047 : d);
    const int s = bit_size(d);
    const unsigned code = kJpegHuffDC[tc][s];
    piece = ((code >> 5) << s) | (unsigned)((d < 0 ? d + (1 << s) - 1 : d) & ((1 << s) - 1));
    plen = (code & 31) + s;
  } else if (nz) {
    const unsigned long long below = mask & ((1ull << lane) - 1);
    const int prev = below ? 63 - __clzll(below) : 0;
    const int run = lane - prev - 1;
    nzrl = run >> 4;
    const int s = bit_size(c);
    const unsigned code = kJpegHuffAC[tc][((run & 15) << 4) | s];
    piece = ((code >> 5) << s) | (unsigned)((c < 0 ? c + (1 << s) - 1 : c) & ((1 << s) - 1));
    plen = (code & 31) + s;
  } else if (lane == 63) {                // the last coefficient is zero: end of block
    const unsigned code = kJpegHuffAC[tc][0];
    piece = code >> 5;
    plen = code & 31;
  }
  const int len = nzrl * zrl_len + plen;
  int incl = len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  const int total = __shfl(incl, 63);
  __syncthreads();
  if (len) {
    unsigned at = incl - len;
    for (int i = 0; i < nzrl; ++i, at += zrl_len) put_bits(words[wave], at, zrl >> 5, zrl_len);
    put_bits(words[wave], at, piece, plen);
  }
  __syncthreads();
  if (valid) {
    if (lane < ((total + 31) >> 5)) a.bits[g * kBlockWords + lane] = words[wave][lane];
    if (lane == 0) a.blen[g] = total;
  }
}

// ---- interval ----------------------------------------------------------------------------------------------------
// exclusive scan of one value per thread over the workgroup; `total` = the sum.  `part`: one cell per wave.
template <int THREADS>
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* part, unsigned& total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  unsigned before = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < THREADS / 64; ++i) {
    const unsigned p = part[i];
    if (i < wave) before += p;
    sum += p;
  }
  __syncthreads();
  total = sum;
  return before + incl - v;
}

__global__ __launch_bounds__(kIntervalThreads) void jpeg_interval_kernel(const JpegArgs a) {
  __shared__ unsigned part[kIntervalThreads / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int nb = a.cols * a.bpm;
  const unsigned* blen = a.blen + (int64_t)r * nb;
  unsigned* boff = a.boff + (int64_t)r * nb;
  const unsigned* bits = a.bits + (int64_t)r * nb * kBlockWords;
  unsigned carry = 0;
  for (int base = 0; base < nb; base += kIntervalThreads) {
    const int j = base + tid;
    unsigned sum;
    const unsigned ex = block_scan<kIntervalThreads>(j < nb ? blen[j] : 0u, part, sum);
    if (j < nb) boff[j] = carry + ex;
    carry += sum;
  }
  __syncthreads();                        // the offsets are read back by the whole workgroup
  const unsigned tb = carry;              // bits of the interval
  const unsigned nbytes = (tb + 7) >> 3, nwords = (nbytes + 3) >> 2;
  unsigned char* out = a.stage + (int64_t)r * a.row_cap;
  unsigned at = 0;                        // stuffed bytes written so far
  for (unsigned base = 0; base < nwords; base += kIntervalThreads) {
    const unsigned wi = base + tid;
    unsigned word = 0xFFFFFFFFu;          // what no block covers is padding
    unsigned nvalid = 0;
    if (wi < nwords) {
      nvalid = nbytes - 4 * wi < 4 ? nbytes - 4 * wi : 4;
      const unsigned p = 32 * wi, pend = p + 32;
      int lo = 0, hi = nb - 1;            // the last block that starts at or before p
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (boff[mid] <= p) lo = mid; else hi = mid - 1;
      }
      unsigned pos = p;
      for (int j = lo; j < nb && pos < pend; ++j) {
        const unsigned start = boff[j], end = start + blen[j];
        if (end <= pos) continue;         // (an empty block cannot occur: every block has at least 4 bits)
        const unsigned o = pos - start;
        const unsigned n = (end < pend ? end : pend) - pos;       // 1..32 bits of block j from its bit o
        const unsigned* bw = bits + (int64_t)j * kBlockWords;
        const unsigned wd = o >> 5, sh = o & 31;
        const unsigned w0 = bw[wd], w1 = (sh + n > 32) ? bw[wd + 1] : 0u;
        const unsigned long long x = ((unsigned long long)w0 << 32 | w1) << sh;
        const unsigned got = (unsigned)(x >> 32) >> (32 - n);     // the n bits, right aligned
        const unsigned shift = pend - pos - n;                    // their place in the word
        const unsigned m = (n == 32 ? 0xFFFFFFFFu : ((1u << n) - 1)) << shift;
        word = (word & ~m) | (got << shift);
        pos += n;
      }
    }
    unsigned nff = 0;
#pragma unroll
    for (unsigned k = 0; k < 4; ++k)
      if (k < nvalid && ((word >> (24 - 8 * k)) & 255u) == 255u) ++nff;
    unsigned sum;
    unsigned o = at + block_scan<kIntervalThreads>(nvalid + nff, part, sum);
#pragma unroll
    for (unsigned k = 0; k < 4; ++k)
      if (k < nvalid) {
        const unsigned byte = (word >> (24 - 8 * k)) & 255u;
        out[o++] = (unsigned char)byte;
        if (byte == 255u) out[o++] = 0;
      }
    at += sum;
  }
  if (tid == 0) {
    if (r != a.rows - 1) {
      out[at] = 0xFF;
      out[at + 1] = (unsigned char)(0xD0 + (r & 7));
      at += 2;
    }
    a.ilen[r] = at;
  }
}

// ---- offsets, compaction -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const JpegArgs a) {
  __shared__ unsigned part[4];
  unsigned carry = 0;
  for (int base = 0; base < a.rows; base += 256) {
    const int j = base + threadIdx.x;
    unsigned sum;
    const unsigned ex = block_scan<256>(j < a.rows ? a.ilen[j] : 0u, part, sum);
    if (j < a.rows) a.ioff[j] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) *a.total = carry;
}

__global__ __launch_bounds__(256) void jpeg_compact_kernel(const JpegArgs a) {
  const int r = blockIdx.y;
  const unsigned n = a.ilen[r];
  const int64_t to = a.ioff[r];
  const unsigned char* src = a.stage + (int64_t)r * a.row_cap;
  for (unsigned i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * 256 * gridDim.x) {
    const unsigned v = *reinterpret_cast<const unsigned*>(src + i);       // row_cap and the area are 4-byte aligned
#pragma unroll
    for (unsigned k = 0; k < 4; ++k)
      if (i + k < n && to + i + k < a.cap) a.scan[to + i + k] = (unsigned char)(v >> (8 * k));
  }
}

struct JpegLayout {
  int rows, cols, bpm, rrows, rcols;
  int64_t blocks, row_cap, coef, bits, blen, boff, stage, ilen, ioff, bytes;
  int64_t scan_max() const { return (int64_t)rows * ((int64_t)cols * bpm * kBlockBytesMax + 2); }   // RSTm after every row
};

bool jpeg_sampling_ok(int sampling) { return sampling == VFML_JPEG_420 || sampling == VFML_JPEG_422 || sampling == VFML_JPEG_444; }

bool jpeg_layout(int h, int w, int sampling, JpegLayout& L) {
  if (h < 1 || w < 1 || h > 65535 || w > 65535 || !jpeg_sampling_ok(sampling)) return false;
  const int mh = sampling == VFML_JPEG_420 ? 16 : 8, mw = sampling == VFML_JPEG_444 ? 8 : 16;
  L.rows = (h + mh - 1) / mh, L.cols = (w + mw - 1) / mw;
  L.bpm = sampling == VFML_JPEG_420 ? 6 : (sampling == VFML_JPEG_422 ? 4 : 3);
  L.rrows = (h + 15) / 16, L.rcols = (w + 15) / 16;
  L.blocks = (int64_t)L.rows * L.cols * L.bpm;
  L.row_cap = align256((int64_t)L.cols * L.bpm * kBlockBytesMax + 2);
  int64_t at = 0;
  L.coef = at, at += align256(L.blocks * 64 * 2);
  L.bits = at, at += align256(L.blocks * kBlockWords * 4);
  L.blen = at, at += align256(L.blocks * 4);
  L.boff = at, at += align256(L.blocks * 4);
  L.stage = at, at += L.rows * L.row_cap;
  L.ilen = at, at += align256(L.rows * 4);
  L.ioff = at, at += align256(L.rows * 4);
  L.bytes = at;
  // the scan's worst case must fit the 32-bit length cell and the 32-bit offsets
  return L.scan_max() <= 0xFFFFFFFFll;
}

template <int S>
void jpeg_launch(const JpegArgs& a, const JpegLayout& L, hipStream_t s) {
  const int64_t nregion = (int64_t)L.rrows * L.rcols;
  hipLaunchKernelGGL(jpeg_transform_kernel<S>, dim3((unsigned)((nregion + 3) / 4)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(jpeg_entropy_kernel<S>, dim3((unsigned)((L.blocks + 3) / 4)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(jpeg_interval_kernel, dim3(L.rows), dim3(kIntervalThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(jpeg_compact_kernel, dim3(32, L.rows), dim3(256), 0, s, a);
}

int jpeg_encode(const char* name, const unsigned char* rgb, int h, int w, int64_t row_stride, int sampling,
                const unsigned char* qtables, void* workspace, unsigned char* scan, int64_t scan_capacity,
                uint32_t* scan_bytes, void* stream) {
  JpegLayout L;
  VFML_REQUIRE(jpeg_sampling_ok(sampling), "%s: sampling %d (VFML_JPEG_420, VFML_JPEG_422 and VFML_JPEG_444 are encoded)", name,
               sampling);
  VFML_REQUIRE(jpeg_layout(h, w, sampling, L), "%s: picture %dx%d (sides of 1..65535, worst-case scan below 4 GiB)", name, w, h);
  VFML_REQUIRE(rgb && qtables && workspace && scan && scan_bytes, "%s: null argument", name);
  VFML_REQUIRE(row_stride >= (int64_t)3 * w, "%s: row stride %lld below the row's %d bytes", name, (long long)row_stride, 3 * w);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace must be 256-byte aligned", name);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(scan_bytes) & 3u) == 0, "%s: scan_bytes must be 4-byte aligned", name);
  VFML_REQUIRE(scan_capacity >= 0, "%s: negative scan capacity", name);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  JpegArgs a;
  a.rgb = rgb, a.h = h, a.w = w, a.stride = row_stride, a.qt = qtables, a.rows = L.rows, a.cols = L.cols;
  a.bpm = L.bpm, a.rrows = L.rrows, a.rcols = L.rcols;
  a.coef = reinterpret_cast<short*>(ws + L.coef);
  a.bits = reinterpret_cast<unsigned*>(ws + L.bits);
  a.blen = reinterpret_cast<unsigned*>(ws + L.blen);
  a.boff = reinterpret_cast<unsigned*>(ws + L.boff);
  a.stage = ws + L.stage, a.row_cap = L.row_cap;
  a.ilen = reinterpret_cast<unsigned*>(ws + L.ilen);
  a.ioff = reinterpret_cast<unsigned*>(ws + L.ioff);
  a.scan = scan, a.cap = scan_capacity, a.total = scan_bytes;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (sampling == VFML_JPEG_420)
    jpeg_launch<0>(a, L, s);
  else if (sampling == VFML_JPEG_422)
    jpeg_launch<1>(a, L, s);
  else
    jpeg_launch<2>(a, L, s);
  return vfml_check_launch(name);
}

}  // namespace

extern "C" int64_t vfml_jpeg_sampled_workspace_bytes(int h, int w, int sampling) {
  JpegLayout L;
  return jpeg_layout(h, w, sampling, L) ? L.bytes : 0;
}

extern "C" int64_t vfml_jpeg_sampled_scan_capacity(int h, int w, int sampling) {
  JpegLayout L;
  return jpeg_layout(h, w, sampling, L) ? L.scan_max() - 2 : 0;
}

extern "C" int vfml_jpeg_encode_rgb_sampled(const unsigned char* rgb, int h, int w, int64_t row_stride, int sampling,
                                            const unsigned char* qtables, void* workspace, unsigned char* scan,
                                            int64_t scan_capacity, uint32_t* scan_bytes, void* stream) {
  return jpeg_encode("vfml_jpeg_encode_rgb_sampled", rgb, h, w, row_stride, sampling, qtables, workspace, scan, scan_capacity,
                     scan_bytes, stream);
}

extern "C" int64_t vfml_jpeg_workspace_bytes(int h, int w) { return vfml_jpeg_sampled_workspace_bytes(h, w, VFML_JPEG_420); }

extern "C" int64_t vfml_jpeg_scan_capacity(int h, int w) { return vfml_jpeg_sampled_scan_capacity(h, w, VFML_JPEG_420); }

extern "C" int vfml_jpeg_encode_rgb(const unsigned char* rgb, int h, int w, int64_t row_stride,
                                    const unsigned char* qtables, void* workspace, unsigned char* scan,
                                    int64_t scan_capacity, uint32_t* scan_bytes, void* stream) {
  return jpeg_encode("vfml_jpeg_encode_rgb", rgb, h, w, row_stride, VFML_JPEG_420, qtables, workspace, scan, scan_capacity,
                     scan_bytes, stream);
}
