// Depthwise k x k convolution over NHWC rows with bias, residual and GELU fused (vfml_dwconv2d), and GELU over rows
// (vfml_gelu_rows): the vector-ALU kernels of the SK ("super kernel") update block.
//
// A depthwise convolution has no reduction over channels: per output it is k * k f32 FMAs with nothing for the matrix
// cores to share.  The kernel is LDS-tiled: a workgroup stages a spatial tile of TH x TW cells with its halo of k / 2 for a
// group of CG = 16 channels as f32 (split rows summed on the way in), the group's weights beside it, and every thread keeps
// a strip of TH = 8 outputs of one column and four channels in registers: per tap column it reads TH + k - 1 cells and the
// k weights of the column once, 16 bytes each, for 8 k float4 FMAs.
//   lanes: t = column * 4 + channel quad; a cell's 16 channels are 64 bytes, so the 16 lanes of a ds_read_b128 group (four
//   columns x four quads) read 256 contiguous bytes = one bank row: no conflicts, no padding.
//   The tap columns are shared between TWO such groups of 128 threads (kx < (k + 1) / 2 and the rest): the tile allows two
//   workgroups per CU, and with one group each that is one wave per SIMD, which cannot hide its own LDS latency.  The groups
//   exchange their partial sums through LDS (over the weights, which are done with by then) and each finishes four of the
//   eight rows: sum = group 0's part + group 1's part, then bias - a fixed order.
//   LDS at k = 15: 22 x 46 cells x 64 B + 16 KiB (225 taps x 64 B, then the exchange) = 81 152 B - two workgroups per CU.
#include "vfml_common.h"

namespace {

constexpr int DW_TH = 8, DW_TW = 32, DW_CG = 16, DW_GROUP = DW_TW * DW_CG / 4, DW_THREADS = 2 * DW_GROUP;
constexpr int DW_EXCHANGE = 2 * (DW_TH / 2) * DW_GROUP * 16;      // bytes: per group, four rows of float4 per thread

template <int K>
constexpr int dw_lds_bytes() {
  const int taps = K * K * DW_CG * 4;
  return (DW_TH + K - 1) * (DW_TW + K - 1) * DW_CG * 4 + (taps > DW_EXCHANGE ? taps : DW_EXCHANGE);
}

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float gelu_exact(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// four channels at channel `col` (a multiple of 4) of a row in either storage format
__device__ __forceinline__ f32x4 load4(const float* row, int col, int fmt) {
  if (fmt == VFML_FMT_S16) {
    const char* u = reinterpret_cast<const char*>(row + (col & ~7)) + (col & 4) * 2;
    const h16x4 hi = *reinterpret_cast<const h16x4*>(u), lo = *reinterpret_cast<const h16x4*>(u + 16);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (float)hi[j] + (float)lo[j];
    return v;
  }
  return *reinterpret_cast<const f32x4*>(row + col);
}

__device__ __forceinline__ void store4(float* row, int col, int fmt, f32x4 v) {
  if (fmt == VFML_FMT_S16) {
    vfml_h16x2 h0, l0, h1, l1;
    vfml_split2(v[0], v[1], h0, l0);
    vfml_split2(v[2], v[3], h1, l1);
    char* u = reinterpret_cast<char*>(row + (col & ~7)) + (col & 4) * 2;
    const h16x4 hi = {h0[0], h0[1], h1[0], h1[1]}, lo = {l0[0], l0[1], l1[0], l1[1]};
    *reinterpret_cast<h16x4*>(u) = hi;
    *reinterpret_cast<h16x4*>(u + 16) = lo;
    return;
  }
  *reinterpret_cast<f32x4*>(row + col) = v;
}

template <int K>
__global__ __launch_bounds__(DW_THREADS) void dwconv_kernel(const float* __restrict__ x, int64_t ld_x, int h, int w, int c,
                                                            const float* __restrict__ weight, const float* __restrict__ bias,
                                                            float* __restrict__ out, int64_t ld_out, int in_fmt, int out_fmt,
                                                            int residual, int act) {
  constexpr int HALO = K / 2, SH = DW_TH + K - 1, SW = DW_TW + K - 1, CG = DW_CG;
  extern __shared__ f32x4 dw_smem[];
  float* tile = reinterpret_cast<float*>(dw_smem);          // [SH][SW][CG]
  float* wl = tile + SH * SW * CG;                          // [K][K][CG]
  const int tid = threadIdx.x;
  const int tiles_x = (w + DW_TW - 1) / DW_TW;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int c0 = blockIdx.y * CG;
  const int64_t frame = blockIdx.z;

  // the group's weights, tap-major: [ky][kx][channel]; channels past c are zero
  for (int i = tid; i < K * K * CG; i += DW_THREADS) {
    const int ch = i / (K * K), t = i - ch * (K * K);
    wl[t * CG + ch] = c0 + ch < c ? weight[(int64_t)c0 * (K * K) + i] : 0.f;
  }
  // the tile with its halo: one 8-channel unit per thread and pass, zero outside the frame
  for (int i = tid; i < SH * SW * 2; i += DW_THREADS) {
    const int u = i & 1, cell = i >> 1;
    const int r = cell / SW, xx = cell - r * SW;
    const int gy = ty * DW_TH + r - HALO, gx = tx * DW_TW + xx - HALO, ch = c0 + u * 8;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (gy >= 0 && gy < h && gx >= 0 && gx < w && ch < c) {
      const float* row = x + ((frame * h + gy) * w + gx) * ld_x;
      if (in_fmt == VFML_FMT_S16) {          // (c % 8 == 0: a whole unit, 16 bytes of hi halves and 16 of lo halves)
        const h16x8 hi = *reinterpret_cast<const h16x8*>(row + ch), lo = *reinterpret_cast<const h16x8*>(row + ch + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = (float)hi[j] + (float)lo[j];
          b[j] = (float)hi[4 + j] + (float)lo[4 + j];
        }
      } else {
        a = *reinterpret_cast<const f32x4*>(row + ch);
        if (ch + 4 < c) b = *reinterpret_cast<const f32x4*>(row + ch + 4);
      }
    }
    *reinterpret_cast<f32x4*>(tile + cell * CG + u * 8) = a;
    *reinterpret_cast<f32x4*>(tile + cell * CG + u * 8 + 4) = b;
  }
  __syncthreads();

  const int grp = tid / DW_GROUP, t = tid % DW_GROUP;
  const int xl = t >> 2, q = t & 3;
  const int kx0 = grp ? (K + 1) / 2 : 0, kx1 = grp ? K : (K + 1) / 2;
  float acc[DW_TH][4];
#pragma unroll
  for (int o = 0; o < DW_TH; ++o)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[o][j] = 0.f;
#pragma unroll 1
  for (int kx = kx0; kx < kx1; ++kx) {
    f32x4 wv[K];
#pragma unroll
    for (int ky = 0; ky < K; ++ky) wv[ky] = *reinterpret_cast<const f32x4*>(wl + (ky * K + kx) * CG + q * 4);
    const float* col = tile + (xl + kx) * CG + q * 4;
#pragma unroll
    for (int r = 0; r < SH; ++r) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(col + r * SW * CG);
#pragma unroll
      for (int o = 0; o < DW_TH; ++o) {
        const int ky = r - o;
        if (ky >= 0 && ky < K) {
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[o][j] = fmaf(wv[ky][j], v[j], acc[o][j]);
        }
      }
    }
  }

  // each group hands the other the partial sums of the four rows that one finishes (group 0: rows 0..3)
  __syncthreads();          // (every thread is done with the weights the exchange overwrites)
  f32x4* part = reinterpret_cast<f32x4*>(wl);
  constexpr int HT = DW_TH / 2;
  float mine[HT][4];
#pragma unroll
  for (int o = 0; o < HT; ++o) {
    f32x4 theirs;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mine[o][j] = grp ? acc[HT + o][j] : acc[o][j];
      theirs[j] = grp ? acc[o][j] : acc[HT + o][j];
    }
    part[(grp * HT + o) * DW_GROUP + t] = theirs;
  }
  __syncthreads();

  const int gx = tx * DW_TW + xl, ch = c0 + q * 4;
  if (gx >= w || ch >= c) return;
  const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + ch);
#pragma unroll
  for (int o = 0; o < HT; ++o) {
    const int row = grp * HT + o, gy = ty * DW_TH + row;
    if (gy >= h) break;
    const f32x4 other = part[((1 - grp) * HT + o) * DW_GROUP + t];
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (grp ? other[j] + mine[o][j] : mine[o][j] + other[j]) + bv[j];
    if (residual) {
      const f32x4 xc = *reinterpret_cast<const f32x4*>(tile + ((row + HALO) * SW + xl + HALO) * CG + q * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += xc[j];
    }
    if (act) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = gelu_exact(v[j]);
    }
    store4(out + ((frame * h + gy) * w + gx) * ld_out, ch, out_fmt, v);
  }
}

// Per-channel affine (k = 1: weight, bias; residual) and / or GELU over rows, four channels per thread and pass.
template <bool AFFINE>
__global__ __launch_bounds__(256) void rows_kernel(const float* x, int64_t ld_x, const float* __restrict__ weight,
                                                   const float* __restrict__ bias, float* out, int64_t ld_out, int64_t rows,
                                                   int c, int in_fmt, int out_fmt, int residual, int act) {
  const int q4 = c / 4;
  const int64_t total = rows * q4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / q4;
    const int col = (int)(i - row * q4) * 4;
    const f32x4 xv = load4(x + row * ld_x, col, in_fmt);
    f32x4 v = xv;
    if constexpr (AFFINE) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(weight + col), bv = *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = fmaf(wv[j], xv[j], bv[j]);
        if (residual) v[j] += xv[j];
      }
    }
    if (act) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = gelu_exact(v[j]);
    }
    store4(out + row * ld_out, col, out_fmt, v);
  }
}

template <int K>
int launch_dwconv(const float* x, int64_t ld_x, int n, int h, int w, int c, const float* weight, const float* bias, float* out,
                  int64_t ld_out, int in_fmt, int out_fmt, int flags, hipStream_t stream) {
  constexpr int lds = dw_lds_bytes<K>();
  static_assert(lds <= 80 * 1024, "two workgroups per CU");
  if (lds > 48 * 1024) {
    const int rc = vfml_lds_cap(reinterpret_cast<const void*>(&dwconv_kernel<K>), lds, "vfml_dwconv2d");
    if (rc) return rc;
  }
  const int64_t tiles = (int64_t)((w + DW_TW - 1) / DW_TW) * ((h + DW_TH - 1) / DW_TH);
  VFML_REQUIRE(tiles < (1ll << 31) && (c + DW_CG - 1) / DW_CG <= 65535 && n <= 65535,
               "vfml_dwconv2d: grid too large (n = %d, c = %d, %lld tiles)", n, c, (long long)tiles);
  hipLaunchKernelGGL(dwconv_kernel<K>, dim3((unsigned)tiles, (c + DW_CG - 1) / DW_CG, n), dim3(DW_THREADS), lds, stream, x, ld_x,
                     h, w, c, weight, bias, out, ld_out, in_fmt, out_fmt, flags & VFML_DW_RESIDUAL, flags & VFML_DW_GELU);
  return vfml_check_launch("vfml_dwconv2d");
}

// shape and alignment of one side's rows; 0 or the reason
const char* rows_fault(const void* p, int64_t ld, int c, int fmt) {
  if (fmt != VFML_FMT_F32 && fmt != VFML_FMT_S16) return "format must be VFML_FMT_F32 or VFML_FMT_S16";
  if (ld < c) return "ld < c";
  if (fmt == VFML_FMT_S16) {
    if (c % 8 || ld % 8 || (reinterpret_cast<uintptr_t>(p) & 31u)) return "misaligned split rows (c and ld multiples of 8, base 32 bytes)";
  } else if (c % 4 || ld % 4 || (reinterpret_cast<uintptr_t>(p) & 15u)) {
    return "misaligned rows (c and ld multiples of 4, base 16 bytes)";
  }
  return nullptr;
}

}  // namespace

extern "C" int vfml_dwconv2d(const float* x, int64_t ld_x, int n, int h, int w, int c, int k, const float* weight,
                             const float* bias, float* out, int64_t ld_out, int in_fmt, int out_fmt, int flags, void* stream) {
  VFML_REQUIRE(x && weight && bias && out, "vfml_dwconv2d: null pointer");
  VFML_REQUIRE(k >= 1 && k <= 15 && (k & 1), "vfml_dwconv2d: k = %d (odd, 1 <= k <= 15)", k);
  VFML_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && (int64_t)n * h * w < (1ll << 31), "vfml_dwconv2d: bad shape n = %d, h = %d, w = %d, c = %d",
               n, h, w, c);
  VFML_REQUIRE((flags & ~(VFML_DW_RESIDUAL | VFML_DW_GELU)) == 0, "vfml_dwconv2d: unknown flags %d", flags);
  const char* why = rows_fault(x, ld_x, c, in_fmt);
  VFML_REQUIRE(!why, "vfml_dwconv2d: x: %s (ld_x = %lld, c = %d)", why, (long long)ld_x, c);
  why = rows_fault(out, ld_out, c, out_fmt);
  VFML_REQUIRE(!why, "vfml_dwconv2d: out: %s (ld_out = %lld, c = %d)", why, (long long)ld_out, c);
  VFML_REQUIRE(vfml_aligned16(weight) && vfml_aligned16(bias), "vfml_dwconv2d: weight and bias must be 16-byte aligned");
  VFML_REQUIRE(static_cast<const void*>(x) != static_cast<const void*>(out),
               "vfml_dwconv2d: in place (out == x) is not supported: a tile's halo is another tile's output");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (k == 1) {
    const int64_t rows = (int64_t)n * h * w, total = rows * (c / 4);
    int64_t g = (total + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(rows_kernel<true>, dim3((unsigned)g), dim3(256), 0, s, x, ld_x, weight, bias, out, ld_out, rows, c, in_fmt,
                       out_fmt, flags & VFML_DW_RESIDUAL, flags & VFML_DW_GELU);
    return vfml_check_launch("vfml_dwconv2d");
  }
  switch (k) {
    case 3: return launch_dwconv<3>(x, ld_x, n, h, w, c, weight, bias, out, ld_out, in_fmt, out_fmt, flags, s);
    case 5: return launch_dwconv<5>(x, ld_x, n, h, w, c, weight, bias, out, ld_out, in_fmt, out_fmt, flags, s);
    case 7: return launch_dwconv<7>(x, ld_x, n, h, w, c, weight, bias, out, ld_out, in_fmt, out_fmt, flags, s);
    case 9: return launch_dwconv<9>(x, ld_x, n, h, w, c, weight, bias, out, ld_out, in_fmt, out_fmt, flags, s);
    case 11: return launch_dwconv<11>(x, ld_x, n, h, w, c, weight, bias, out, ld_out, in_fmt, out_fmt, flags, s);
    case 13: return launch_dwconv<13>(x, ld_x, n, h, w, c, weight, bias, out, ld_out, in_fmt, out_fmt, flags, s);
    default: return launch_dwconv<15>(x, ld_x, n, h, w, c, weight, bias, out, ld_out, in_fmt, out_fmt, flags, s);
  }
}

extern "C" int vfml_gelu_rows(const float* x, int64_t ld_x, float* out, int64_t ld_out, int64_t rows, int c, int in_fmt,
                              int out_fmt, void* stream) {
  VFML_REQUIRE(x && out, "vfml_gelu_rows: null pointer");
  VFML_REQUIRE(rows > 0 && rows < (1ll << 31) && c > 0, "vfml_gelu_rows: bad shape rows = %lld, c = %d", (long long)rows, c);
  const char* why = rows_fault(x, ld_x, c, in_fmt);
  VFML_REQUIRE(!why, "vfml_gelu_rows: x: %s (ld_x = %lld, c = %d)", why, (long long)ld_x, c);
  why = rows_fault(out, ld_out, c, out_fmt);
  VFML_REQUIRE(!why, "vfml_gelu_rows: out: %s (ld_out = %lld, c = %d)", why, (long long)ld_out, c);
  VFML_REQUIRE(static_cast<const void*>(x) != static_cast<const void*>(out) || (in_fmt == out_fmt && ld_x == ld_out),
               "vfml_gelu_rows: in place needs the same format and row stride on both sides");
  const int64_t total = rows * (c / 4);
  int64_t g = (total + 255) / 256;
  if (g > 16384) g = 16384;
  hipLaunchKernelGGL(rows_kernel<false>, dim3((unsigned)g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, ld_x,
                     nullptr, nullptr, out, ld_out, rows, c, in_fmt, out_fmt, 0, 1);
  return vfml_check_launch("vfml_gelu_rows");
}
