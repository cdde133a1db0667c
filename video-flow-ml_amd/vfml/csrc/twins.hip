// The three kernels of the Twins-SVT encoders: LayerNorm over rows (vfml_layernorm_rows), the
// locally-grouped attention of a 7 x 7 window (vfml_window_attention) and the attention of many queries against one frame's
// sub-sampled keys (vfml_attention_shared_keys).  Head dimension 32 throughout; rows in either storage format.
//
// vfml_attention_shared_keys is the hot one (1080p: 129 600 queries x 1 980 keys x 4 heads, 2 x 2 p pk d FLOP per head) and
// runs on the f32 matrix cores, v_mfma_f32_32x32x2_f32, with an online softmax - no score ever reaches memory:
//   a workgroup is four waves = 128 queries of one (frame, head); a chunk of 128 keys and values is staged in LDS as f32 and
//   shared by the four waves; a wave owns 32 queries and walks the chunk in tiles of 32 keys.
//   Scores are computed TRANSPOSED, S^T = K Q^T (A = keys from LDS, B = the wave's queries, held in 16 registers for the
//   whole kernel): the accumulator then holds, per lane, 16 keys of ONE query (column = lane % 32), so the running maximum
//   and sum are per-lane scalars (one exchange with lane ^ 32), and exp(S^T - m) is already in the B-operand layout of the
//   second product O^T = V^T P^T - accumulator register r of lane l is key 8 (r / 4) + 4 (l / 32) + r % 4, and a sum over
//   keys may take them in any order as long as the A operand (V^T, read from LDS) takes the same one.  No register
//   transposes, no LDS round trip of the probabilities: 32 MFMAs and 32 ds_read_b32 per tile and wave.
//   LDS: keys [128][33] (odd stride: the 32 lanes of an A-operand read take 32 keys of one dimension) + values [128][32]
//   = 33 280 B, four workgroups per CU.
#include "vfml_common.h"

namespace {

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

constexpr int HD = 32;      // head dimension: the only one built

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

// ----------------------------------------------------------------------------------------------------- LayerNorm
// A row is held by G = 16, 32 or 64 lanes, eight channels per lane and pass, at most LN_U passes: read once, mean first,
// then the variance of x - mean (no E[x^2] - E[x]^2 cancellation), both folded over the G lanes by butterflies.
constexpr int LN_U = 4, LN_MAX_C = 64 * 8 * LN_U;

template <int G>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* x, int64_t ld_x, float* out, int64_t ld_out, int64_t rows,
                                                        int c, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, int in_fmt, int out_fmt) {
  const int lane = threadIdx.x % G;
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  const bool live = row < rows;
  const float* xr = x + (live ? row : 0) * ld_x;
  float v[LN_U][8];
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < LN_U; ++u) {
    const int col = (u * G + lane) * 8;
    if (col < c) {
      const f32x4 a = load4(xr, col, in_fmt), b = load4(xr, col + 4, in_fmt);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[u][j] = a[j];
        v[u][4 + j] = b[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[u][j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += v[u][j];
  }
#pragma unroll
  for (int m = G / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, G);
  const float mean = sum / (float)c;
  float sq = 0.f;
#pragma unroll
  for (int u = 0; u < LN_U; ++u) {
    if ((u * G + lane) * 8 < c) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[u][j] -= mean;
        sq = fmaf(v[u][j], v[u][j], sq);
      }
    }
  }
#pragma unroll
  for (int m = G / 2; m >= 1; m >>= 1) sq += __shfl_xor(sq, m, G);
  const float rstd = 1.0f / sqrtf(sq / (float)c + eps);
  if (!live) return;
  float* orow = out + row * ld_out;
#pragma unroll
  for (int u = 0; u < LN_U; ++u) {
    const int col = (u * G + lane) * 8;
    if (col < c) {
#pragma unroll
      for (int hlf = 0; hlf < 2; ++hlf) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + col + 4 * hlf), b = *reinterpret_cast<const f32x4*>(beta + col + 4 * hlf);
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = fmaf(v[u][4 * hlf + j] * rstd, g[j], b[j]);
        store4(orow, col + 4 * hlf, out_fmt, y);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------- window attention
// One wave per (frame, window, head): keys and values of the window's 49 tokens in LDS, lane i < 49 owns query i.  Pass 1
// writes the lane's 49 scores to LDS (column = lane: conflict free) and keeps their maximum, pass 2 sums exp(s - max) and
// the weighted values.  Keys and values are read as broadcasts (every lane the same address).
constexpr int WS = 7, WT = WS * WS;
constexpr int WA_LDS_FLOATS = 2 * WT * HD + WT * 64;

__global__ __launch_bounds__(64) void window_attention_kernel(const float* __restrict__ qkv, int64_t ld, int h, int w, int c,
                                                              int heads, const float* __restrict__ pad_row, float* __restrict__ out,
                                                              int64_t ld_out, int in_fmt, int out_fmt, float scale) {
  __shared__ f32x4 wa_smem[WA_LDS_FLOATS / 4];
  float* kl = reinterpret_cast<float*>(wa_smem);     // [49][32]
  float* vl = kl + WT * HD;                          // [49][32]
  float* sc = vl + WT * HD;                          // [49][64]
  const int lane = threadIdx.x;
  const int wins_x = (w + WS - 1) / WS;
  const int head = blockIdx.x % heads, win = blockIdx.x / heads;
  const int wx = win % wins_x, wy = win / wins_x;
  const int64_t frame = blockIdx.y;
  const int col0 = head * HD;

  // keys and values: 49 tokens x 2 x 8 quads
  for (int i = lane; i < WT * 16; i += 64) {
    const int tok = i >> 4, part = i & 15, which = part >> 3, quad = part & 7;
    const int y = wy * WS + tok / WS, xx = wx * WS + tok % WS;
    const int col = (1 + which) * c + col0 + quad * 4;
    f32x4 t;
    if (y < h && xx < w)
      t = load4(qkv + ((frame * h + y) * w + xx) * ld, col, in_fmt);
    else
      t = *reinterpret_cast<const f32x4*>(pad_row + col);
    *reinterpret_cast<f32x4*>((which ? vl : kl) + tok * HD + quad * 4) = t;
  }
  // the lane's query, straight into registers
  const int tq = lane < WT ? lane : WT - 1;
  const int qy = wy * WS + tq / WS, qx = wx * WS + tq % WS;
  const bool inside = qy < h && qx < w;
  float q[HD];
#pragma unroll
  for (int j = 0; j < HD / 4; ++j) {
    f32x4 t;
    if (inside)
      t = load4(qkv + ((frame * h + qy) * w + qx) * ld, col0 + j * 4, in_fmt);
    else
      t = *reinterpret_cast<const f32x4*>(pad_row + col0 + j * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) q[j * 4 + e] = t[e] * scale;
  }
  __syncthreads();

  float mx = -INFINITY;
#pragma unroll 1
  for (int t = 0; t < WT; ++t) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < HD / 4; ++j) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(kl + t * HD + j * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(q[j * 4 + e], kv[e], s);
    }
    sc[t * 64 + lane] = s;
    mx = fmaxf(mx, s);
  }
  float acc[HD];
#pragma unroll
  for (int j = 0; j < HD; ++j) acc[j] = 0.f;
  float sum = 0.f;
#pragma unroll 1
  for (int t = 0; t < WT; ++t) {
    const float p = expf(sc[t * 64 + lane] - mx);      // (the lane's own column: written by itself above)
    sum += p;
#pragma unroll
    for (int j = 0; j < HD / 4; ++j) {
      const f32x4 vv = *reinterpret_cast<const f32x4*>(vl + t * HD + j * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j * 4 + e] = fmaf(p, vv[e], acc[j * 4 + e]);
    }
  }
  if (lane >= WT || !inside) return;
  const float inv = 1.0f / sum;
  float* orow = out + ((frame * h + qy) * w + qx) * ld_out;
#pragma unroll
  for (int j = 0; j < HD / 4; ++j) {
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = acc[j * 4 + e] * inv;
    store4(orow, col0 + j * 4, out_fmt, y);
  }
}

// ----------------------------------------------------------------------------------------------------- shared-key attention
constexpr int SK_WAVES = 4, SK_THREADS = 64 * SK_WAVES, SK_QW = 32, SK_QB = SK_QW * SK_WAVES;
constexpr int SK_CHUNK = 128, SK_KLD = HD + 1;

__global__ __launch_bounds__(SK_THREADS) void attention_shared_keys_kernel(const float* __restrict__ q, int64_t ld_q,
                                                                           const float* __restrict__ kv, int64_t ld_kv, int p, int pk,
                                                                           int c, float* __restrict__ out, int64_t ld_out, int q_fmt,
                                                                           int kv_fmt, int out_fmt, float scale) {
  __shared__ float kl[SK_CHUNK * SK_KLD];       // keys   [chunk][33]
  __shared__ f32x4 vl4[SK_CHUNK * HD / 4];      // values [chunk][32]
  float* vl = reinterpret_cast<float*>(vl4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, half = lane >> 5;
  const int head = blockIdx.y;
  const int64_t frame = blockIdx.z;
  const int col0 = head * HD;
  const int q0 = blockIdx.x * SK_QB + wave * SK_QW;
  const int qi = q0 + l32;
  const int qrow = qi < p ? qi : p - 1;          // (ragged last block: a valid row is read, nothing is stored)

  // B operand of S^T = K Q^T, fixed for the kernel: step t takes dimensions t (lanes 0..31) and 16 + t (lanes 32..63)
  float qreg[16];
  {
    const float* qr = q + (frame * p + qrow) * ld_q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 t = load4(qr, col0 + half * 16 + j * 4, q_fmt);
#pragma unroll
      for (int e = 0; e < 4; ++e) qreg[j * 4 + e] = t[e];
    }
  }
  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  float mrun = -INFINITY, lrun = 0.f;

  for (int k0 = 0; k0 < pk; k0 += SK_CHUNK) {
    __syncthreads();          // (the last chunk's readers are done)
    // stage the chunk: 128 keys x (8 key quads + 8 value quads), zero behind the last key
    for (int i = tid; i < SK_CHUNK * 16; i += SK_THREADS) {
      const int key = i >> 4, part = i & 15, which = part >> 3, quad = part & 7;
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (k0 + key < pk) t = load4(kv + (frame * pk + k0 + key) * ld_kv, which * c + col0 + quad * 4, kv_fmt);
      if (which) {
        *reinterpret_cast<f32x4*>(vl + key * HD + quad * 4) = t;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) kl[key * SK_KLD + quad * 4 + e] = t[e];
      }
    }
    __syncthreads();
    const int left = pk - k0;
    const int tiles = left >= SK_CHUNK ? SK_CHUNK / 32 : (left + 31) / 32;
#pragma unroll 1
    for (int tl = 0; tl < tiles; ++tl) {
      const int kb = tl * 32;
      // S^T[key][query]: A = K[kb + l32][t + 16 half]
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int t = 0; t < 16; ++t)
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kl[(kb + l32) * SK_KLD + t + 16 * half], qreg[t], s, 0, 0, 0);
      // register r of this lane: key kb + 8 (r / 4) + 4 half + r % 4, query l32
      float mt = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + kb + 8 * (r >> 2) + 4 * half + (r & 3);
        s[r] = key < pk ? s[r] * scale : -INFINITY;
        mt = fmaxf(mt, s[r]);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float mnew = fmaxf(mrun, mt);          // (finite: every tile walked has a key below pk)
      const float alpha = expf(mrun - mnew);
      float ls = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = expf(s[r] - mnew);
        ls += s[r];
        o[r] *= alpha;
      }
      ls += __shfl_xor(ls, 32, 64);
      lrun = fmaf(lrun, alpha, ls);
      mrun = mnew;
      // O^T[d][query] += V^T P^T: step r sums keys kb + 8 (r / 4) + r % 4 (k = 0) and that + 4 (k = 1); A = V[key][d = l32]
#pragma unroll
      for (int r = 0; r < 16; ++r)
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(vl[(kb + 8 * (r >> 2) + 4 * half + (r & 3)) * HD + l32], s[r], o, 0, 0, 0);
    }
  }
  if (qi >= p) return;
  const float inv = 1.0f / lrun;
  float* orow = out + (frame * p + qi) * ld_out;
  // register r: dimension 8 (r / 4) + 4 half + r % 4 of query l32
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = o[a * 4 + e] * inv;
    store4(orow, col0 + 8 * a + 4 * half, out_fmt, y);
  }
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

extern "C" int vfml_layernorm_rows(const float* x, int64_t ld_x, float* out, int64_t ld_out, int64_t rows, int c, const float* gamma,
                                   const float* beta, float eps, int in_fmt, int out_fmt, void* stream) {
  VFML_REQUIRE(x && out && gamma && beta, "vfml_layernorm_rows: null pointer");
  VFML_REQUIRE(rows > 0 && rows < (1ll << 31) && c > 0 && c % 8 == 0 && c <= LN_MAX_C,
               "vfml_layernorm_rows: bad shape rows = %lld, c = %d (c a multiple of 8, at most %d)", (long long)rows, c, LN_MAX_C);
  VFML_REQUIRE(eps > 0.f, "vfml_layernorm_rows: eps = %g", (double)eps);
  const char* why = rows_fault(x, ld_x, c, in_fmt);
  VFML_REQUIRE(!why, "vfml_layernorm_rows: x: %s (ld_x = %lld, c = %d)", why, (long long)ld_x, c);
  why = rows_fault(out, ld_out, c, out_fmt);
  VFML_REQUIRE(!why, "vfml_layernorm_rows: out: %s (ld_out = %lld, c = %d)", why, (long long)ld_out, c);
  VFML_REQUIRE(vfml_aligned16(gamma) && vfml_aligned16(beta), "vfml_layernorm_rows: gamma and beta must be 16-byte aligned");
  VFML_REQUIRE(static_cast<const void*>(x) != static_cast<const void*>(out) || ld_x == ld_out,
               "vfml_layernorm_rows: in place needs the same row stride on both sides");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int units = c / 8;
  const int g = units <= 16 ? 16 : units <= 32 ? 32 : 64;
  const int64_t blocks = (rows * g + 255) / 256;
  VFML_REQUIRE(blocks < (1ll << 31), "vfml_layernorm_rows: grid too large (%lld rows)", (long long)rows);
#define VFML_LN_LAUNCH(G)                                                                                                      \
  hipLaunchKernelGGL(layernorm_kernel<G>, dim3((unsigned)blocks), dim3(256), 0, s, x, ld_x, out, ld_out, rows, c, gamma, beta, \
                     eps, in_fmt, out_fmt)
  if (g == 16)
    VFML_LN_LAUNCH(16);
  else if (g == 32)
    VFML_LN_LAUNCH(32);
  else
    VFML_LN_LAUNCH(64);
#undef VFML_LN_LAUNCH
  return vfml_check_launch("vfml_layernorm_rows");
}

extern "C" int vfml_window_attention(const float* qkv, int64_t ld, int n, int h, int w, int c, int heads, int ws,
                                     const float* pad_row, float* out, int64_t ld_out, int in_fmt, int out_fmt, void* stream) {
  VFML_REQUIRE(qkv && pad_row && out, "vfml_window_attention: null pointer");
  VFML_REQUIRE(ws == WS, "vfml_window_attention: ws = %d (7 is the only window size built)", ws);
  VFML_REQUIRE(n > 0 && h > 0 && w > 0 && (int64_t)n * h * w < (1ll << 31), "vfml_window_attention: bad shape n = %d, h = %d, w = %d",
               n, h, w);
  VFML_REQUIRE(heads > 0 && c > 0 && c == heads * HD, "vfml_window_attention: c = %d is not heads * 32 (heads = %d)", c, heads);
  VFML_REQUIRE(ld >= 3 * (int64_t)c, "vfml_window_attention: qkv: ld < 3 c (ld = %lld, c = %d)", (long long)ld, c);
  const char* why = rows_fault(qkv, ld, 3 * c, in_fmt);
  VFML_REQUIRE(!why, "vfml_window_attention: qkv: %s (ld = %lld, c = %d)", why, (long long)ld, c);
  why = rows_fault(out, ld_out, c, out_fmt);
  VFML_REQUIRE(!why, "vfml_window_attention: out: %s (ld_out = %lld, c = %d)", why, (long long)ld_out, c);
  VFML_REQUIRE(vfml_aligned16(pad_row), "vfml_window_attention: pad_row must be 16-byte aligned");
  VFML_REQUIRE(static_cast<const void*>(qkv) != static_cast<const void*>(out), "vfml_window_attention: in place (out == qkv) is not supported");
  const int64_t blocks = (int64_t)((h + WS - 1) / WS) * ((w + WS - 1) / WS) * heads;
  VFML_REQUIRE(blocks < (1ll << 31) && n <= 65535, "vfml_window_attention: grid too large (n = %d, %lld window heads)", n,
               (long long)blocks);
  hipLaunchKernelGGL(window_attention_kernel, dim3((unsigned)blocks, n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), qkv, ld,
                     h, w, c, heads, pad_row, out, ld_out, in_fmt, out_fmt, 1.0f / sqrtf((float)HD));
  return vfml_check_launch("vfml_window_attention");
}

extern "C" int vfml_attention_shared_keys(const float* q, int64_t ld_q, const float* kv, int64_t ld_kv, int n, int p, int pk, int c,
                                          int heads, float* out, int64_t ld_out, int q_fmt, int kv_fmt, int out_fmt, void* stream) {
  VFML_REQUIRE(q && kv && out, "vfml_attention_shared_keys: null pointer");
  VFML_REQUIRE(n > 0 && p > 0 && (int64_t)n * p < (1ll << 31), "vfml_attention_shared_keys: bad shape n = %d, p = %d", n, p);
  VFML_REQUIRE(pk > 0 && (int64_t)n * pk < (1ll << 31), "vfml_attention_shared_keys: pk = %d (at least one key)", pk);
  VFML_REQUIRE(heads > 0 && c > 0 && c == heads * HD, "vfml_attention_shared_keys: c = %d is not heads * 32 (heads = %d)", c, heads);
  const char* why = rows_fault(q, ld_q, c, q_fmt);
  VFML_REQUIRE(!why, "vfml_attention_shared_keys: q: %s (ld_q = %lld, c = %d)", why, (long long)ld_q, c);
  VFML_REQUIRE(ld_kv >= 2 * (int64_t)c, "vfml_attention_shared_keys: kv: ld < 2 c (ld_kv = %lld, c = %d)", (long long)ld_kv, c);
  why = rows_fault(kv, ld_kv, 2 * c, kv_fmt);
  VFML_REQUIRE(!why, "vfml_attention_shared_keys: kv: %s (ld_kv = %lld, c = %d)", why, (long long)ld_kv, c);
  why = rows_fault(out, ld_out, c, out_fmt);
  VFML_REQUIRE(!why, "vfml_attention_shared_keys: out: %s (ld_out = %lld, c = %d)", why, (long long)ld_out, c);
  VFML_REQUIRE(static_cast<const void*>(q) != static_cast<const void*>(out) && static_cast<const void*>(kv) != static_cast<const void*>(out),
               "vfml_attention_shared_keys: in place (out == q or kv) is not supported");
  VFML_REQUIRE(heads <= 65535 && n <= 65535, "vfml_attention_shared_keys: grid too large (n = %d, heads = %d)", n, heads);
  hipLaunchKernelGGL(attention_shared_keys_kernel, dim3((unsigned)((p + SK_QB - 1) / SK_QB), heads, n), dim3(SK_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), q, ld_q, kv, ld_kv, p, pk, c, out, ld_out, q_fmt, kv_fmt, out_fmt,
                     1.0f / sqrtf((float)HD));
  return vfml_check_launch("vfml_attention_shared_keys");
}
