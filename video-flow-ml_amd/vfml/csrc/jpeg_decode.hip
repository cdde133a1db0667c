// vfml_jpeg_decode_rgb, vfml_jpeg_decode_rgb_sampled: the decoder of the MJPG frames the drop-in reads (DESIGN.md
// sections 13 and 13.2) - baseline sequential DCT, 8-bit, YCbCr 4:2:0, 4:2:2 or 4:4:4 in one interleaved scan or one grey
// component, any Huffman tables, any restart interval.  Integer arithmetic only: T.81 F.2.2 entropy decoding, libjpeg's
// jidctint "islow" inverse DCT, its h2v2 / h2v1 "fancy" chroma upsampling and its colour conversion, so the picture equals
// libjpeg's byte for byte; tests/jpeg_decode_oracle.py (4:2:0) and tests/jpeg_sampling_oracle.py are the same definition
// in numpy.  The sampling sets the blocks of an MCU (DecArgs nb, ny: uniform values of the entropy stages) and
// instantiates the transform and the colour kernel.
// The marker segments are read on the host (storage/jpeg_parse.py); nothing on the host looks at the entropy data.
//
// Five launches on one stream, no synchronisation:
//   count      every thread tests 16 byte pairs of the scan for FF D0..D7; one count per 4096-byte chunk.
//   place      the counts before a chunk and a workgroup scan give every marker its rank: the byte ranges of the
//              intervals, in order, without atomics.  The number of markers and their sequence m = 0, 1, ... modulo 8
//              are checked into the status cell.
//   entropy    one restart interval per wave64 (the unit of parallelism the format gives).  The wave stages the
//              interval's bytes in an LDS ring, 256 at a time, the stuffed 00s removed by ballot and prefix count; the
//              symbol chain is serial, its values wave-uniform: a code's length is the first lane whose left-aligned
//              code limit exceeds the next 16 bits (one ballot), its symbol one LDS read.  A block is built in LDS and
//              stored by all lanes, int16 in natural order, nb (six in 4:2:0) per MCU.
//   transform  one wave per MCU: dequantisation, then a lane per column and a lane per row of its blocks for the two
//              IDCT passes through LDS; 8-bit Y, Cb, Cr planes of the padded size in the workspace.
//   colour     a lane per chroma sample of an output row: the triangle filter and the conversion of its two pixels
//              (4:4:4 and grey: a lane per pixel, no filter).
// Bounds on a damaged stream: interval ranges are clamped to the scan, the ring is indexed modulo its size, a block reads
// at most 64 symbols of at most 31 bits (less than the 320 bytes staged ahead), a coefficient index is checked against
// 63 before it is used, table indices are masked to the table.  What is wrong ends in the status cell, and nothing is
// written outside the workspace and the output rows.
// jpeg_decode_sync.hip is the same decoder with another entropy stage (a lane per subsequence of the scan, for files
// whose intervals are long or missing); it launches count / place and transform / colour through jpeg_decode_common.h.
#include "jpeg_decode_common.h"

using namespace vfml_jpeg;

namespace {

#include "jpeg_tables.inc"

constexpr int kRing = 1024;               // bytes of an interval staged in LDS (a power of two)
constexpr int kStageAhead = 320;          // staged before a block: 64 symbols of 31 bits are 248 bytes, + the bit buffer

// ---- markers -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_rst(const DecArgs& a, unsigned p) {
  return p + 1 < a.n && a.scan[p] == 0xFF && (a.scan[p + 1] & 0xF8) == 0xD0;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// the sum of one value per thread over the workgroup of kChunkThreads, and each thread's exclusive prefix
__device__ __forceinline__ unsigned chunk_scan(unsigned v, unsigned* part, unsigned& total) {
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
  for (int i = 0; i < kChunkThreads / 64; ++i) {
    const unsigned p = part[i];
    if (i < wave) before += p;
    sum += p;
  }
  __syncthreads();
  total = sum;
  return before + incl - v;
}

__device__ __forceinline__ unsigned count_markers(const DecArgs& a, unsigned base) {
  unsigned c = 0;
  for (unsigned k = 0; k < 16; ++k) c += is_rst(a, base + k) ? 1u : 0u;
  return c;
}

__global__ __launch_bounds__(kChunkThreads) void jpeg_dec_count_kernel(const DecArgs a) {
  __shared__ unsigned part[kChunkThreads / 64];
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.status = 0;
  const unsigned base = blockIdx.x * (unsigned)kChunk + threadIdx.x * 16u;
  unsigned total;
  chunk_scan(count_markers(a, base), part, total);
  if (threadIdx.x == 0) a.bcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(kChunkThreads) void jpeg_dec_place_kernel(const DecArgs a) {
  __shared__ unsigned part[kChunkThreads / 64];
  unsigned before = 0;                    // markers in the chunks in front of this one
  for (unsigned i = threadIdx.x; i < blockIdx.x; i += kChunkThreads) before += a.bcount[i];
  unsigned sum;
  chunk_scan(before, part, sum);
  before = sum;
  const unsigned base = blockIdx.x * (unsigned)kChunk + threadIdx.x * 16u;
  unsigned total;
  unsigned rank = before + chunk_scan(count_markers(a, base), part, total);
  for (unsigned k = 0; k < 16; ++k)
    if (is_rst(a, base + k)) {
      if (rank + 1 < (unsigned)a.nint) a.mpos[rank] = base + k;
      if ((unsigned)(a.scan[base + k + 1] & 7) != (rank & 7u)) atomicOr(a.status, kErrSequence);
      ++rank;
    }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && before + total + 1 != (unsigned)a.nint)
    atomicOr(a.status, kErrCount);
}

// ---- entropy -----------------------------------------------------------------------------------------------------
struct BitReader {
  unsigned long long acc;                 // the next bits, most significant first
  int nb;                                 // how many of them are valid
  unsigned rd;                            // bytes taken from the ring (a multiple of 4)
};

__device__ __forceinline__ void fill(BitReader& br, const unsigned* ring) {
  if (br.nb <= 32) {
    const unsigned v = __builtin_bswap32(ring[(br.rd >> 2) & (kRing / 4 - 1)]);
    br.acc |= (unsigned long long)v << (32 - br.nb);
    br.nb += 32;
    br.rd += 4;
  }
}

// s (1..15) value bits, EXTENDed (T.81 F.2.2.1)
__device__ __forceinline__ int receive_extend(BitReader& br, int s) {
  const int v = (int)(br.acc >> (64 - s));
  br.acc <<= s;
  br.nb -= s;
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

__global__ __launch_bounds__(64) void jpeg_dec_entropy_kernel(const DecArgs a) {
  __shared__ unsigned ring[kRing / 4];
  __shared__ int valoff[4][16];
  __shared__ unsigned huffval[4][64];     // 256 bytes per table
  __shared__ unsigned char zigzag[64];
  __shared__ short blk[64];
  const int lane = threadIdx.x;
  if (*a.status != 0) return;             // a wrong interval count or sequence: the ranges mean nothing
  const int it = a.int0 + blockIdx.x;
  // the tables: limits in registers (lane l: codes of l + 1 bits), offsets and symbols in LDS
  int lim[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    lim[t] = lane < 16 ? a.tables[8 + 96 * t + lane] : 0;
    huffval[t][lane] = (unsigned)a.tables[8 + 96 * t + 32 + lane];
  }
  valoff[lane >> 4][lane & 15] = a.tables[8 + 96 * (lane >> 4) + 16 + (lane & 15)];
  zigzag[lane] = kJpegZigzag[lane];
  int dc_t[3], ac_t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) dc_t[c] = a.tables[2 * c] & 3, ac_t[c] = a.tables[2 * c + 1] & 3;
  // the interval's bytes, clamped to the scan
  unsigned src = it == 0 ? 0u : a.mpos[it - 1] + 2u;
  unsigned end = it == a.nint - 1 ? a.n : a.mpos[it];
  src = src < a.n ? src : a.n;
  end = end < src ? src : (end < a.n ? end : a.n);
  const int nmcu = a.rows * a.cols;
  const int m0 = it * a.ri;
  const int m1 = m0 + a.ri < nmcu ? m0 + a.ri : nmcu;
  unsigned wr = 0;                        // bytes staged so far (stuffing removed)
  unsigned carry = 0;                     // the raw byte in front of the next one to stage
  BitReader br = {0ull, 0, 0u};
  int pred0 = 0, pred1 = 0, pred2 = 0;
  int err = 0;
  const unsigned char* huffbytes = reinterpret_cast<const unsigned char*>(&huffval[0][0]);
  unsigned char* ringbytes = reinterpret_cast<unsigned char*>(ring);
  __syncthreads();
  for (int mcu = m0; mcu < m1 && !err; ++mcu) {
    for (int b = 0; b < a.nb && !err; ++b) {
      // stage ahead: 256 raw bytes per step, four loads in flight
      while (wr - br.rd < (unsigned)kStageAhead && src < end) {
        unsigned raw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned p = src + 64 * j + lane;
          raw[j] = p < end ? a.scan[p] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned p = src + 64 * j + lane;
          unsigned prev = __shfl_up(raw[j], 1);
          if (lane == 0) prev = carry;
          const bool keep = p < end && !(raw[j] == 0u && prev == 0xFFu);
          const unsigned long long mask = __ballot(keep);
          const unsigned off = __popcll(mask & ((1ull << lane) - 1ull));
          if (keep) ringbytes[(wr + off) & (kRing - 1)] = (unsigned char)raw[j];
          wr += __popcll(mask);
          carry = __shfl(raw[j], 63);
        }
        src += 256;
      }
      blk[lane] = 0;
      __syncthreads();
      const int comp = b < a.ny ? 0 : b - a.ny + 1;
      // DC
      {
        const int t = dc_t[comp];
        fill(br, ring);
        const int v = (int)(br.acc >> 48);
        const int lt = t == 0 ? lim[0] : t == 1 ? lim[1] : t == 2 ? lim[2] : lim[3];
        const unsigned long long m = __ballot(lane < 16 && v < lt);
        if (m == 0ull) {
          err = kErrCode;
          break;
        }
        const int l = __ffsll((long long)m);
        const int s = huffbytes[t * 256 + ((valoff[t][l - 1] + (v >> (16 - l))) & 255)] & 15;
        br.acc <<= l;
        br.nb -= l;
        int pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
        if (s) pred += receive_extend(br, s);
        if (comp == 0) pred0 = pred; else if (comp == 1) pred1 = pred; else pred2 = pred;
        if (lane == 0) blk[0] = (short)pred;
      }
      // AC
      {
        const int t = ac_t[comp];
        const int lt = t == 0 ? lim[0] : t == 1 ? lim[1] : t == 2 ? lim[2] : lim[3];
        int k = 1;
        while (k < 64) {
          fill(br, ring);
          const int v = (int)(br.acc >> 48);
          const unsigned long long m = __ballot(lane < 16 && v < lt);
          if (m == 0ull) {
            err = kErrCode;
            break;
          }
          const int l = __ffsll((long long)m);
          const int rs = huffbytes[t * 256 + ((valoff[t][l - 1] + (v >> (16 - l))) & 255)];
          br.acc <<= l;
          br.nb -= l;
          const int r = rs >> 4, s = rs & 15;
          if (s == 0) {
            if (r != 15) break;           // EOB
            if (k + 16 > 64) {
              err = kErrIndex;
              break;
            }
            k += 16;                      // ZRL
            continue;
          }
          k += r;
          if (k > 63) {
            err = kErrIndex;
            break;
          }
          const int val = receive_extend(br, s);
          if (lane == 0) blk[zigzag[k]] = (short)val;
          ++k;
        }
      }
      if (!err && src >= end && 8ull * br.rd - (unsigned)br.nb > 8ull * wr) err = kErrData;
      __syncthreads();
      if (!err) a.coef[((int64_t)mcu * a.nb + b) * 64 + lane] = blk[lane];
      __syncthreads();
    }
  }
  if (err && lane == 0) atomicOr(a.status, err);
}

// ---- transform ---------------------------------------------------------------------------------------------------
// libjpeg jidctint's 1-D pass over i[0..7], without the final descale
__device__ __forceinline__ void idct_butterfly(const int* i, int* o) {
  int z1 = (i[2] + i[6]) * 4433;
  const int t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
  const int t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int p = i[7], q = i[5], r = i[3], s = i[1];
  z1 = p + s;
  int z2 = q + r, z3 = p + r, z4 = q + s;
  const int z5 = (z3 + z4) * 9633;
  p *= 2446, q *= 16819, r *= 25172, s *= 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  p += z1 + z3, q += z2 + z4, r += z2 + z3, s += z1 + z4;
  o[0] = t10 + s, o[7] = t10 - s, o[1] = t11 + r, o[6] = t11 - r;
  o[2] = t12 + q, o[5] = t12 - q, o[3] = t13 + p, o[4] = t13 - p;
}

// S: the sampling.  A wave per MCU: lanes 0 .. 8 nb - 1 take a column, then a row, of its nb blocks.
template <int S>
__global__ __launch_bounds__(256) void jpeg_dec_transform_kernel(const DecArgs a) {
  constexpr int NB = samp_nb(S), NY = samp_ny(S), HS = samp_hs(S), VS = samp_vs(S);
  __shared__ int ws[4][NB][64 + 8];       // a row of 9: the column pass and the row pass both spread over the banks
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int count = a.mrows * a.cols;
  int g = blockIdx.x * 4 + wave;
  const bool valid = g < count;
  if (!valid) g = count - 1;
  const int mcu = a.mrow0 * a.cols + g;
  const int my = mcu / a.cols, mx = mcu - my * a.cols;
  const int at = (lane >> 3) * 9 + (lane & 7);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int comp = b < NY ? 0 : b - NY + 1;
    ws[wave][b][at] = (int)a.coef[((int64_t)mcu * NB + b) * 64 + lane] * (int)a.qt[comp * 64 + lane];
  }
  __syncthreads();
  const int b = lane >> 3, j = lane & 7;  // lanes 0 .. 8 NB - 1: block b, column / row j
  int in[8], out[8];
  if (lane < 8 * NB) {
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = ws[wave][b][r * 9 + j];
    idct_butterfly(in, out);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[wave][b][r * 9 + j] = (out[r] + 1024) >> 11;
  }
  __syncthreads();
  if (lane < 8 * NB) {
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = ws[wave][b][j * 9 + c];
    idct_butterfly(in, out);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      int v = ((out[c] + (1 << 17)) >> 18) + 128;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      if (c < 4) lo |= (unsigned)v << (8 * c); else hi |= (unsigned)v << (8 * (c - 4));
    }
    if (valid) {
      unsigned char* dst;
      if (b < NY)
        dst = a.py + ((int64_t)my * (8 * VS) + (b / HS) * 8 + j) * (a.cols * (8 * HS)) + mx * (8 * HS) + (b % HS) * 8;
      else
        dst = (b == NY ? a.pcb : a.pcr) + ((int64_t)my * 8 + j) * (a.cols * 8) + mx * 8;
      *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);     // planes are 256-byte aligned, their rows multiples of 8
    }
  }
}

// ---- colour ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned char clamp255(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__device__ __forceinline__ void store_rgb(unsigned char* dst, int Y, int cb, int cr) {
  dst[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
  dst[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  dst[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

// 4:2:2: a lane per chroma sample of an output row and its two pixels: libjpeg's h2v1 triangle filter, which it uses
// where the chroma plane is more than 2 samples wide; a narrower one has every sample repeated
__global__ __launch_bounds__(256) void jpeg_dec_colour422_kernel(const DecArgs a) {
  const int cw = (a.w + 1) >> 1;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cw) return;
  const int y = a.y0 + blockIdx.y;
  const int cl = c > 0 ? c - 1 : 0, cr_ = c < cw - 1 ? c + 1 : cw - 1;
  int even[2], odd[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const unsigned char* p0 = (k == 0 ? a.pcb : a.pcr) + (int64_t)y * (a.cols * 8);
    const int s = p0[c];
    even[k] = (cw > 2 ? (3 * s + p0[cl] + 1) >> 2 : s) - 128;
    odd[k] = (cw > 2 ? (3 * s + p0[cr_] + 2) >> 2 : s) - 128;
  }
  const unsigned char* yrow = a.py + (int64_t)y * (a.cols * 16);
  unsigned char* dst = a.rgb + (int64_t)blockIdx.y * a.stride + 6 * (int64_t)c;
  store_rgb(dst, yrow[2 * c], even[0], even[1]);
  if (2 * c + 1 < a.w) store_rgb(dst + 3, yrow[2 * c + 1], odd[0], odd[1]);
}

// 4:4:4 and grey: a lane per pixel; no filter, and for grey no chroma: R = G = B = Y
template <bool Grey>
__global__ __launch_bounds__(256) void jpeg_dec_colour11_kernel(const DecArgs a) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= a.w) return;
  const int y = a.y0 + blockIdx.y;
  const int64_t at = (int64_t)y * (a.cols * 8) + x;
  unsigned char* dst = a.rgb + (int64_t)blockIdx.y * a.stride + 3 * (int64_t)x;
  const int Y = a.py[at];
  if (Grey) {
    dst[0] = dst[1] = dst[2] = (unsigned char)Y;
  } else {
    store_rgb(dst, Y, (int)a.pcb[at] - 128, (int)a.pcr[at] - 128);
  }
}

__global__ __launch_bounds__(256) void jpeg_dec_colour_kernel(const DecArgs a) {
  const int ch = (a.h + 1) >> 1, cw = (a.w + 1) >> 1;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cw) return;
  const int y = a.y0 + blockIdx.y;
  const int r = y >> 1;
  int nb = (y & 1) ? r + 1 : r - 1;
  nb = nb < 0 ? 0 : (nb > ch - 1 ? ch - 1 : nb);
  const int cl = c > 0 ? c - 1 : 0, cr_ = c < cw - 1 ? c + 1 : cw - 1;
  const int pw = a.cols * 8;
  int even[2], odd[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const unsigned char* p = k == 0 ? a.pcb : a.pcr;
    const unsigned char* p0 = p + (int64_t)r * pw;
    const unsigned char* p1 = p + (int64_t)nb * pw;
    const int s = 3 * p0[c] + p1[c], sl = 3 * p0[cl] + p1[cl], sr = 3 * p0[cr_] + p1[cr_];
    even[k] = ((3 * s + sl + 8) >> 4) - 128;
    odd[k] = ((3 * s + sr + 7) >> 4) - 128;
  }
  const unsigned char* yrow = a.py + (int64_t)y * (a.cols * 16);
  unsigned char* dst = a.rgb + (int64_t)blockIdx.y * a.stride + 6 * (int64_t)c;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int x = 2 * c + k;
    if (x >= a.w) break;
    const int Y = yrow[x];
    const int cb = k ? odd[0] : even[0], cr = k ? odd[1] : even[1];
    dst[3 * k] = clamp255(Y + ((91881 * cr + 32768) >> 16));
    dst[3 * k + 1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    dst[3 * k + 2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
  }
}

}  // namespace

void vfml_jpeg::dec_launch_markers(const DecArgs& a, unsigned chunks, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_dec_count_kernel, dim3(chunks), dim3(kChunkThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_dec_place_kernel, dim3(chunks), dim3(kChunkThreads), 0, s, a);
}

void vfml_jpeg::dec_launch_picture(const DecArgs& a, hipStream_t s) {
  const dim3 tg((unsigned)((a.mrows * a.cols + 3) / 4)), rows1(1, (unsigned)(a.y1 - a.y0));
  const dim3 half((unsigned)(((a.w + 1) / 2 + 255) / 256), rows1.y), full((unsigned)((a.w + 255) / 256), rows1.y);
  switch (a.samp) {
    case kS420:
      hipLaunchKernelGGL(jpeg_dec_transform_kernel<kS420>, tg, dim3(256), 0, s, a);
      hipLaunchKernelGGL(jpeg_dec_colour_kernel, half, dim3(256), 0, s, a);
      break;
    case kS422:
      hipLaunchKernelGGL(jpeg_dec_transform_kernel<kS422>, tg, dim3(256), 0, s, a);
      hipLaunchKernelGGL(jpeg_dec_colour422_kernel, half, dim3(256), 0, s, a);
      break;
    case kS444:
      hipLaunchKernelGGL(jpeg_dec_transform_kernel<kS444>, tg, dim3(256), 0, s, a);
      hipLaunchKernelGGL(jpeg_dec_colour11_kernel<false>, full, dim3(256), 0, s, a);
      break;
    default:
      hipLaunchKernelGGL(jpeg_dec_transform_kernel<kSGrey>, tg, dim3(256), 0, s, a);
      hipLaunchKernelGGL(jpeg_dec_colour11_kernel<true>, full, dim3(256), 0, s, a);
      break;
  }
}

extern "C" int64_t vfml_jpeg_decode_sampled_workspace_bytes(int h, int w, int sampling, int64_t scan_bytes) {
  DecLayout L;
  return dec_layout(h, w, sampling, scan_bytes, L) ? L.bytes : 0;
}

extern "C" int64_t vfml_jpeg_decode_workspace_bytes(int h, int w, int64_t scan_bytes) {
  return vfml_jpeg_decode_sampled_workspace_bytes(h, w, kS420, scan_bytes);
}

// fn: the entry point's name, for its messages
static int decode_rgb(const char* fn, const unsigned char* scan, int64_t scan_bytes, int h, int w, int sampling,
                      int restart_interval, const unsigned char* qtables, const int32_t* tables, int y0, int y1,
                      void* workspace, unsigned char* rgb, int64_t row_stride, int32_t* status, void* stream) {
  VFML_REQUIRE(samp_ok(sampling), "%s: sampling %d (VFML_JPEG_420, _422, _444 or _GREY)", fn, sampling);
  DecLayout L;
  VFML_REQUIRE(dec_layout(h, w, sampling, scan_bytes, L), "%s: picture %dx%d, scan of %lld bytes (sides of 1..65535, "
               "a scan below 2 GiB)", fn, w, h, (long long)scan_bytes);
  VFML_REQUIRE(scan && qtables && tables && workspace && rgb && status, "%s: null argument", fn);
  VFML_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, "%s: restart interval %d", fn, restart_interval);
  VFML_REQUIRE(0 <= y0 && y0 < y1 && y1 <= h, "%s: rows %d..%d of a picture of %d", fn, y0, y1, h);
  VFML_REQUIRE(row_stride >= (int64_t)3 * w, "%s: row stride %lld below the row's %d bytes", fn, (long long)row_stride,
               3 * w);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace must be 256-byte aligned", fn);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(tables) & 3u) == 0 && (reinterpret_cast<uintptr_t>(status) & 3u) == 0,
               "%s: tables and status must be 4-byte aligned", fn);
  DecArgs a;
  dec_args(a, L, static_cast<unsigned char*>(workspace), scan, scan_bytes, h, w, sampling, restart_interval, qtables,
           tables, y0, y1, rgb, row_stride, status);
  const int mlo = a.mrow0, mhi = a.mrow0 + a.mrows - 1;
  int ilo = 0, ihi = a.nint - 1;          // intervals are skipped when each is a whole number of MCU rows
  if (restart_interval > 0 && restart_interval % L.cols == 0) {
    const int k = restart_interval / L.cols;
    ilo = mlo / k, ihi = mhi / k;
  }
  a.int0 = ilo;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  dec_launch_markers(a, (unsigned)L.chunks, s);
  hipLaunchKernelGGL(jpeg_dec_entropy_kernel, dim3((unsigned)(ihi - ilo + 1)), dim3(64), 0, s, a);
  dec_launch_picture(a, s);
  return vfml_check_launch(fn);
}

extern "C" int vfml_jpeg_decode_rgb_sampled(const unsigned char* scan, int64_t scan_bytes, int h, int w, int sampling,
                                            int restart_interval, const unsigned char* qtables, const int32_t* tables,
                                            int y0, int y1, void* workspace, unsigned char* rgb, int64_t row_stride,
                                            int32_t* status, void* stream) {
  return decode_rgb("vfml_jpeg_decode_rgb_sampled", scan, scan_bytes, h, w, sampling, restart_interval, qtables, tables, y0,
                    y1, workspace, rgb, row_stride, status, stream);
}

extern "C" int vfml_jpeg_decode_rgb(const unsigned char* scan, int64_t scan_bytes, int h, int w, int restart_interval,
                                    const unsigned char* qtables, const int32_t* tables, int y0, int y1, void* workspace,
                                    unsigned char* rgb, int64_t row_stride, int32_t* status, void* stream) {
  return decode_rgb("vfml_jpeg_decode_rgb", scan, scan_bytes, h, w, kS420, restart_interval, qtables, tables, y0, y1,
                    workspace, rgb, row_stride, status, stream);
}
