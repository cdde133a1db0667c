// The attention plane of the GMA aggregator in one call: plane[i][j] = f16(prob_scale * softmax_j(score_scale * q_i . k_j)),
// from f32 q / k rows straight to the f16 plane the read-out GEMM takes as its weight (hip.PlainWeight).  The P x P scores
// never reach memory: pass 1 forms every score tile on the matrix cores and keeps each row's running maximum and sum (online
// softmax) - 2 p floats of workspace -, pass 2 forms the tiles again and stores the probabilities.
//
// Arithmetic: both operands as split f16 (hi + lo of 16 x) and three MFMAs per product (lo.hi, hi.lo, hi.hi) in BOTH passes -
// the scores then carry about 22 bits; a pass on hi halves alone would move them by ~3e-3 for unit-variance operands, ten
// times the 2^-12 the f16 plane itself carries.  |16 x| must stay inside f16 (|x| < 4094).
//
// Shape: a workgroup of four waves owns 128 queries, 32 per wave, held for the whole pass as the B operand of
// v_mfma_f32_32x32x16_f16 (8 k-steps x (hi, lo) = 64 VGPRs).  The keys stream through LDS 64 at a time: loaded as f32 (the next
// tile's loads are in flight while the current one is multiplied), split once per workgroup, read back as A fragments.  With
// the keys as A a lane's 16 accumulators are 16 keys of ONE query (column = lane & 31), so maximum, sum and exponentials are
// per-lane work; the two lane halves of a query are joined once, after the last tile.
#include "vfml_common.h"

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

constexpr int ATT_D = 128;          // channels of q and k (the only value built)
constexpr int ATT_BM = 128;         // queries per workgroup
constexpr int ATT_BN = 64;          // keys per LDS stage
constexpr int ATT_LD = ATT_D + 8;   // LDS row of halves: 272 bytes, 16 lanes' ds_read_b128 cover all 64 banks
constexpr float ATT_IN_SCALE = 16.0f;   // power of two: exact; keeps the lo halves of O(1) operands normal

__device__ __forceinline__ void att_split4(f32x4 v, h16x4& h, h16x4& l) {
  vfml_h16x2 h0, l0, h1, l1;
  vfml_split2(v[0] * ATT_IN_SCALE, v[1] * ATT_IN_SCALE, h0, l0);
  vfml_split2(v[2] * ATT_IN_SCALE, v[3] * ATT_IN_SCALE, h1, l1);
  h = h16x4{h0[0], h0[1], h1[0], h1[1]};
  l = h16x4{l0[0], l0[1], l1[0], l1[1]};
}

// PASS 1: stats[row] = max_j t_ij, stats[p + row] = sum_j 2^(t_ij - max), t = log2(e) * score_scale * q.k
// PASS 2: plane[row][j] = f16(prob_scale * 2^(t_ij - max) / sum), zero for p <= j < ld_plane
template <int PASS>
__global__ __launch_bounds__(256) void attention_plane_kernel(const float* __restrict__ q, int64_t ld_q,
                                                              const float* __restrict__ k, int64_t ld_k, int p, float t_scale,
                                                              float prob_scale, _Float16* __restrict__ plane, int64_t ld_plane,
                                                              float* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) _Float16 khi[ATT_BN][ATT_LD];
  __shared__ __attribute__((aligned(16))) _Float16 klo[ATT_BN][ATT_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, half = lane >> 5;
  const int row = blockIdx.x * ATT_BM + wave * 32 + r;       // this lane's query
  const float NEG_INF = -__builtin_inff();

  // the wave's queries as B fragments: lane (r, half) holds q[row][16 s + 8 half + 0..7] of k-step s
  h16x8 qhi[8], qlo[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
    if (row < p) {
      const float* src = q + (int64_t)row * ld_q + 16 * s + 8 * half;
      a = *reinterpret_cast<const f32x4*>(src);
      b = *reinterpret_cast<const f32x4*>(src + 4);
    }
    h16x4 ha, la, hb, lb;
    att_split4(a, ha, la);
    att_split4(b, hb, lb);
    qhi[s] = __builtin_shufflevector(ha, hb, 0, 1, 2, 3, 4, 5, 6, 7);
    qlo[s] = __builtin_shufflevector(la, lb, 0, 1, 2, 3, 4, 5, 6, 7);
  }

  float m = NEG_INF, l = 0.f, inv = 0.f;
  if (PASS == 2 && row < p) {
    m = stats[row];
    inv = prob_scale / stats[p + row];
  }

  // pass 1 needs the tiles that hold a key; pass 2 also writes the zeros of the row stride (ld_plane % 64 == 0)
  const int ntiles = PASS == 1 ? (p + ATT_BN - 1) / ATT_BN : (int)(ld_plane / ATT_BN);
  f32x4 stage[8];       // the next tile's keys: thread t holds float4 (t + 256 n) of [64 keys][32 float4]
  auto fetch = [&](int tile) {
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int i = t + 256 * n, kr = tile * ATT_BN + (i >> 5);
      stage[n] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kr < p) stage[n] = *reinterpret_cast<const f32x4*>(k + (int64_t)kr * ld_k + 4 * (i & 31));
    }
  };
  fetch(0);
  for (int tile = 0; tile < ntiles; ++tile) {
    __syncthreads();          // the previous tile's fragments have been read
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int i = t + 256 * n;
      h16x4 h, lo;
      att_split4(stage[n], h, lo);
      *reinterpret_cast<h16x4*>(&khi[i >> 5][4 * (i & 31)]) = h;
      *reinterpret_cast<h16x4*>(&klo[i >> 5][4 * (i & 31)]) = lo;
    }
    __syncthreads();
    if (tile + 1 < ntiles) fetch(tile + 1);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        // A fragments: lane (r, half) holds key (32 sub + r), channels 16 s + 8 half + 0..7
        const h16x8 ah = *reinterpret_cast<const h16x8*>(&khi[32 * sub + r][16 * s + 8 * half]);
        const h16x8 al = *reinterpret_cast<const h16x8*>(&klo[32 * sub + r][16 * s + 8 * half]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, qhi[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qlo[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qhi[s], acc, 0, 0, 0);
      }
      // acc[e]: query = this lane's, key = key0 + (e & 3) + 8 (e >> 2) + 4 half
      const int key0 = tile * ATT_BN + 32 * sub + 4 * half;
      float tv[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = key0 + (e & 3) + 8 * (e >> 2);
        tv[e] = key < p ? acc[e] * t_scale : NEG_INF;
      }
      if (PASS == 1) {
        float mx = tv[0];
#pragma unroll
        for (int e = 1; e < 16; ++e) mx = fmaxf(mx, tv[e]);
        const float mn = fmaxf(m, mx);
        const float ms = mn == NEG_INF ? 0.f : mn;       // (no key of this lane half yet: every term below is 2^-inf = 0)
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) sum += __builtin_amdgcn_exp2f(tv[e] - ms);
        l = l * __builtin_amdgcn_exp2f(m - ms) + sum;
        m = mn;
      } else if (row < p) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          h16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (_Float16)(__builtin_amdgcn_exp2f(tv[4 * g + e] - m) * inv);
          *reinterpret_cast<h16x4*>(plane + (int64_t)row * ld_plane + key0 + 8 * g) = o;
        }
      }
    }
  }
  if (PASS == 1) {
    // the two lane halves of a query hold disjoint keys: join them
    const float mo = __shfl_xor(m, 32), lo = __shfl_xor(l, 32);
    const float mn = fmaxf(m, mo);
    const float ms = mn == NEG_INF ? 0.f : mn;
    const float sum = l * __builtin_amdgcn_exp2f(m - ms) + lo * __builtin_amdgcn_exp2f(mo - ms);
    if (half == 0 && row < p) {
      stats[row] = mn;
      stats[p + row] = sum;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The bank form (MemFlow's memory): the queries of one frame against n_seg key sets of p rows each - the keys of earlier
// fields and the frame's own -, softmax JOINTLY over all n_seg * p columns, written as n_seg planes [p][ld_plane], plane s
// holding the columns of key set s.  The same kernel shape and arithmetic as above; the tile walk runs over (set, tile)
// pairs, and a set's last tile is partial whenever p % 64 != 0: its dead keys are -inf (probability 0), in both passes.
constexpr int ATT_MAX_SEG = 9;

struct att_bank_args {
  const float* k[ATT_MAX_SEG];
  _Float16* plane[ATT_MAX_SEG];
};

template <int PASS>
__global__ __launch_bounds__(256) void attention_bank_kernel(const float* __restrict__ q, int64_t ld_q, att_bank_args bank,
                                                             int64_t ld_k, int n_seg, int p, float t_scale, float prob_scale,
                                                             int64_t ld_plane, float* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) _Float16 khi[ATT_BN][ATT_LD];
  __shared__ __attribute__((aligned(16))) _Float16 klo[ATT_BN][ATT_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, half = lane >> 5;
  const int row = blockIdx.x * ATT_BM + wave * 32 + r;       // this lane's query
  const float NEG_INF = -__builtin_inff();

  h16x8 qhi[8], qlo[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
    if (row < p) {
      const float* src = q + (int64_t)row * ld_q + 16 * s + 8 * half;
      a = *reinterpret_cast<const f32x4*>(src);
      b = *reinterpret_cast<const f32x4*>(src + 4);
    }
    h16x4 ha, la, hb, lb;
    att_split4(a, ha, la);
    att_split4(b, hb, lb);
    qhi[s] = __builtin_shufflevector(ha, hb, 0, 1, 2, 3, 4, 5, 6, 7);
    qlo[s] = __builtin_shufflevector(la, lb, 0, 1, 2, 3, 4, 5, 6, 7);
  }

  float m = NEG_INF, l = 0.f, inv = 0.f;
  if (PASS == 2 && row < p) {
    m = stats[row];
    inv = prob_scale / stats[p + row];
  }

  // tiles of one key set: pass 1 those that hold a key, pass 2 the whole row stride (the zeros of p .. ld_plane-1)
  const int tps = PASS == 1 ? (p + ATT_BN - 1) / ATT_BN : (int)(ld_plane / ATT_BN);
  f32x4 stage[8];
  auto fetch = [&](int seg, int tile) {
    const float* __restrict__ ks = bank.k[seg];          // (seg is uniform: a scalar load from the kernel arguments)
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int i = t + 256 * n, kr = tile * ATT_BN + (i >> 5);
      stage[n] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kr < p) stage[n] = *reinterpret_cast<const f32x4*>(ks + (int64_t)kr * ld_k + 4 * (i & 31));
    }
  };
  fetch(0, 0);
  for (int seg = 0; seg < n_seg; ++seg) {
    _Float16* __restrict__ plane = PASS == 2 ? bank.plane[seg] : nullptr;
    for (int tile = 0; tile < tps; ++tile) {
      __syncthreads();          // the previous tile's fragments have been read
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const int i = t + 256 * n;
        h16x4 h, lo;
        att_split4(stage[n], h, lo);
        *reinterpret_cast<h16x4*>(&khi[i >> 5][4 * (i & 31)]) = h;
        *reinterpret_cast<h16x4*>(&klo[i >> 5][4 * (i & 31)]) = lo;
      }
      __syncthreads();
      if (tile + 1 < tps) fetch(seg, tile + 1);
      else if (seg + 1 < n_seg) fetch(seg + 1, 0);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const h16x8 ah = *reinterpret_cast<const h16x8*>(&khi[32 * sub + r][16 * s + 8 * half]);
          const h16x8 al = *reinterpret_cast<const h16x8*>(&klo[32 * sub + r][16 * s + 8 * half]);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, qhi[s], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qlo[s], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qhi[s], acc, 0, 0, 0);
        }
        // acc[e]: query = this lane's, key (within the set) = key0 + (e & 3) + 8 (e >> 2)
        const int key0 = tile * ATT_BN + 32 * sub + 4 * half;
        float tv[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = key0 + (e & 3) + 8 * (e >> 2);
          tv[e] = key < p ? acc[e] * t_scale : NEG_INF;
        }
        if (PASS == 1) {
          float mx = tv[0];
#pragma unroll
          for (int e = 1; e < 16; ++e) mx = fmaxf(mx, tv[e]);
          const float mn = fmaxf(m, mx);
          const float ms = mn == NEG_INF ? 0.f : mn;
          float sum = 0.f;
#pragma unroll
          for (int e = 0; e < 16; ++e) sum += __builtin_amdgcn_exp2f(tv[e] - ms);
          l = l * __builtin_amdgcn_exp2f(m - ms) + sum;
          m = mn;
        } else if (row < p) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            h16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (_Float16)(__builtin_amdgcn_exp2f(tv[4 * g + e] - m) * inv);
            *reinterpret_cast<h16x4*>(plane + (int64_t)row * ld_plane + key0 + 8 * g) = o;
          }
        }
      }
    }
  }
  if (PASS == 1) {
    const float mo = __shfl_xor(m, 32), lo = __shfl_xor(l, 32);
    const float mn = fmaxf(m, mo);
    const float ms = mn == NEG_INF ? 0.f : mn;
    const float sum = l * __builtin_amdgcn_exp2f(m - ms) + lo * __builtin_amdgcn_exp2f(mo - ms);
    if (half == 0 && row < p) {
      stats[row] = mn;
      stats[p + row] = sum;
    }
  }
}

// y += scale * x, n floats in float4s
__global__ void axpy_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n4, float scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + 4 * i);
    f32x4 yv = *reinterpret_cast<const f32x4*>(y + 4 * i);
    yv[0] += scale * xv[0];
    yv[1] += scale * xv[1];
    yv[2] += scale * xv[2];
    yv[3] += scale * xv[3];
    *reinterpret_cast<f32x4*>(y + 4 * i) = yv;
  }
}

}  // namespace

extern "C" int vfml_attention_bank_planes_f16(const float* q, int64_t ld_q, const float* const* keys, int64_t ld_k, int n_seg,
                                              int p, int d, float score_scale, float prob_scale, void* const* planes,
                                              int64_t ld_plane, void* workspace, void* stream) {
  VFML_REQUIRE(q && keys && planes && workspace, "vfml_attention_bank_planes_f16: null pointer");
  VFML_REQUIRE(n_seg >= 1 && n_seg <= ATT_MAX_SEG, "vfml_attention_bank_planes_f16: n_seg = %d out of 1..%d", n_seg,
               ATT_MAX_SEG);
  VFML_REQUIRE(d == ATT_D, "vfml_attention_bank_planes_f16: d = %d, built for d = %d only", d, ATT_D);
  VFML_REQUIRE(p > 0, "vfml_attention_bank_planes_f16: p = %d", p);
  VFML_REQUIRE(ld_plane % 64 == 0 && ld_plane >= p && ld_plane <= 32768,
               "vfml_attention_bank_planes_f16: ld_plane = %lld: a multiple of 64, p <= ld_plane <= 32768",
               (long long)ld_plane);
  VFML_REQUIRE(ld_q >= d && ld_k >= d && ld_q % 4 == 0 && ld_k % 4 == 0 && vfml_aligned16(q),
               "vfml_attention_bank_planes_f16: q / k rows of whole, 16-byte aligned float4s (ld >= d, ld %% 4 == 0)");
  att_bank_args bank = {};
  for (int s = 0; s < n_seg; ++s) {
    VFML_REQUIRE(keys[s] && planes[s], "vfml_attention_bank_planes_f16: null pointer (key set / plane %d)", s);
    VFML_REQUIRE(vfml_aligned16(keys[s]) && vfml_aligned16(planes[s]),
                 "vfml_attention_bank_planes_f16: key set / plane %d must be 16-byte aligned", s);
    bank.k[s] = keys[s];
    bank.plane[s] = (_Float16*)planes[s];
  }
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "vfml_attention_bank_planes_f16: workspace 4-byte aligned");
  VFML_REQUIRE(score_scale == score_scale && score_scale - score_scale == 0.f,
               "vfml_attention_bank_planes_f16: score_scale %g is not a finite number", (double)score_scale);
  VFML_REQUIRE(prob_scale >= 1.0f && prob_scale <= 32768.0f,
               "vfml_attention_bank_planes_f16: prob_scale %g out of [1, 2^15]", (double)prob_scale);
  const float t_scale = score_scale * 1.44269504088896340736f / (ATT_IN_SCALE * ATT_IN_SCALE);
  const dim3 grid((p + ATT_BM - 1) / ATT_BM), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(attention_bank_kernel<1>, grid, block, 0, st, q, ld_q, bank, ld_k, n_seg, p, t_scale, prob_scale, ld_plane,
                     (float*)workspace);
  hipLaunchKernelGGL(attention_bank_kernel<2>, grid, block, 0, st, q, ld_q, bank, ld_k, n_seg, p, t_scale, prob_scale, ld_plane,
                     (float*)workspace);
  return vfml_check_launch("vfml_attention_bank_planes_f16");
}

extern "C" int vfml_axpy_f32(const float* x, float* y, int64_t n, float scale, void* stream) {
  VFML_REQUIRE(x && y && n > 0 && n % 4 == 0, "vfml_axpy_f32: bad argument (n %% 4 == 0)");
  VFML_REQUIRE(vfml_aligned16(x) && vfml_aligned16(y), "vfml_axpy_f32: x and y must be 16-byte aligned");
  int64_t g = (n / 4 + 255) / 256;
  if (g > 16384) g = 16384;
  hipLaunchKernelGGL(axpy_f32_kernel, dim3((unsigned)g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y, n / 4, scale);
  return vfml_check_launch("vfml_axpy_f32");
}

extern "C" int64_t vfml_attention_plane_workspace_bytes(int p) { return p > 0 ? 2 * (int64_t)p * (int64_t)sizeof(float) : 0; }

extern "C" int vfml_attention_plane_f16(const float* q, int64_t ld_q, const float* k, int64_t ld_k, int p, int d,
                                        float score_scale, float prob_scale, void* plane, int64_t ld_plane, void* workspace,
                                        void* stream) {
  VFML_REQUIRE(q && k && plane && workspace, "vfml_attention_plane_f16: null pointer");
  VFML_REQUIRE(d == ATT_D, "vfml_attention_plane_f16: d = %d, built for d = %d only", d, ATT_D);
  VFML_REQUIRE(p > 0, "vfml_attention_plane_f16: p = %d", p);
  VFML_REQUIRE(ld_plane % 64 == 0 && ld_plane >= p && ld_plane <= 32768,
               "vfml_attention_plane_f16: ld_plane = %lld: a multiple of 64, p <= ld_plane <= 32768", (long long)ld_plane);
  VFML_REQUIRE(ld_q >= d && ld_k >= d && ld_q % 4 == 0 && ld_k % 4 == 0 && vfml_aligned16(q) && vfml_aligned16(k),
               "vfml_attention_plane_f16: q / k rows of whole, 16-byte aligned float4s (ld >= d, ld %% 4 == 0)");
  VFML_REQUIRE(vfml_aligned16(plane) && (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0,
               "vfml_attention_plane_f16: plane must be 16-byte aligned, workspace 4-byte");
  VFML_REQUIRE(score_scale == score_scale && score_scale - score_scale == 0.f,
               "vfml_attention_plane_f16: score_scale %g is not a finite number", (double)score_scale);
  VFML_REQUIRE(prob_scale >= 1.0f && prob_scale <= 32768.0f, "vfml_attention_plane_f16: prob_scale %g out of [1, 2^15]",
               (double)prob_scale);
  // scores in log2 units (2^t = e^score), with the operands' factor 16 x 16 taken out
  const float t_scale = score_scale * 1.44269504088896340736f / (ATT_IN_SCALE * ATT_IN_SCALE);
  const dim3 grid((p + ATT_BM - 1) / ATT_BM), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(attention_plane_kernel<1>, grid, block, 0, st, q, ld_q, k, ld_k, p, t_scale, prob_scale,
                     (_Float16*)plane, ld_plane, (float*)workspace);
  hipLaunchKernelGGL(attention_plane_kernel<2>, grid, block, 0, st, q, ld_q, k, ld_k, p, t_scale, prob_scale,
                     (_Float16*)plane, ld_plane, (float*)workspace);
  return vfml_check_launch("vfml_attention_plane_f16");
}
