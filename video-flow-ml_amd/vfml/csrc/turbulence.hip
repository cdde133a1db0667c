// Turbulence map of a flow field (reference flow_visualizer.py: generate_turbulence_map :2997-3052):
// a JET heat map of the local standard deviation of the flow vectors, normalised between the 5th and 95th percentile
// of the frame.  DESIGN.md section 10 defines every rounding step.  Launches, all on the caller's stream:
//   1. hipMemsetAsync           the three histogram levels
//   2. turbulence_moments       per 32x64 tile: the (resized) field with its k/2 halo staged in LDS as f32, BORDER_REFLECT
//                               applied on the way in; k x k box sums of x, y, x*x, y*y in f64 (columns first, then rows, in
//                               strips of 4 output rows); tv = sqrt(max(0, var_x) + max(0, var_y)) written once, and a
//                               histogram of the top 11 bits of its bit pattern (tv >= +0: the u32 pattern orders as the
//                               float does)
//   3. select<1>                one block, one wave per wanted order statistic: the bin its rank falls in
//   4. refine_hist<2>           the next 11 bits of the values inside those bins
//   5. select<2>
//   6. refine_hist<3>           the last 10 bits
//   7. select<3>                the four values, numpy's lerp of each pair -> lo, hi
//   8. turbulence_colour        normalise, index, JET
// The selection is integer counting only: exact, and the same bytes on every run.
#include "vfml_common.h"

namespace {

constexpr int TH = 32, TW = 64, SR = 4, NT = 256;   // tile, rows per strip, threads (SR * TW == NT)
constexpr int BITS1 = 11, BITS2 = 11, BITS3 = 10;
constexpr int BINS1 = 1 << BITS1, BINS2 = 1 << BITS2, BINS3 = 1 << BITS3;
constexpr int MAX_RADIUS = 31;

__device__ const unsigned JET[256] = {
#include "jet_table.inc"
};

// Device-side state of the selection: per wanted order statistic the bit prefix found so far, the rank left inside it,
// and the first statistic that shares the prefix (its histogram row serves both).
struct SelState {
  unsigned prefix[4], rank[4], own[4];
  float lohi[2];
};

struct Workspace {        // byte offsets into the caller's workspace
  size_t hist1, hist2, hist3, state, tv, total;
};

inline Workspace layout(int64_t n) {
  Workspace ws;
  ws.hist1 = 0;
  ws.hist2 = ws.hist1 + sizeof(unsigned) * BINS1;
  ws.hist3 = ws.hist2 + sizeof(unsigned) * 4 * BINS2;
  ws.state = ws.hist3 + sizeof(unsigned) * 4 * BINS3;
  ws.tv = (ws.state + sizeof(SelState) + 255) / 256 * 256;
  ws.total = ws.tv + sizeof(float) * (size_t)n;
  return ws;
}

struct MomentArgs {
  const float* flow; float* tv; unsigned* hist;
  int h, w, fh, fw, radius, resize;
  int tiles_x;
  float scale_y, scale_x, mul_x, mul_y;
  double inv_area;          // 1.0 / (k * k)
};

__device__ __forceinline__ float root32(float x) { return (float)sqrt((double)x); }   // correctly rounded
__device__ __forceinline__ float div32(float x, float y) { return (float)((double)x / (double)y); }

// A staged vector read from LDS whose first readers are 32-bit moves: the conversions to f64 that follow take a 64-bit
// register pair, and no such op of this library is the first reader of an LDS result (vfml_common.h: vfml_lds_f64).
__device__ __forceinline__ float2 lds_f32x2(const float2* p) {
  const float2 v = *p;
  float2 r;
  asm("v_mov_b32 %0, %1" : "=v"(r.x) : "v"(v.x));
  asm("v_mov_b32 %0, %1" : "=v"(r.y) : "v"(v.y));
  return r;
}

// BORDER_REFLECT (fedcba|abcdefgh|hgfedcb), periodic when the image is shorter than the reach
__device__ __forceinline__ int reflect(int p, int n) {
  const int period = 2 * n;
  int q = p % period;
  if (q < 0) q += period;
  return q < n ? q : period - 1 - q;
}

// source taps of one output coordinate of the bilinear resize: csrc/effects.hip taps()
__device__ __forceinline__ void taps(int dst, float scale, int n_in, int& i0, int& i1, float& l0, float& l1) {
  float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
  src = fmaxf(src, 0.0f);
  i0 = min((int)floorf(src), n_in - 1);
  i0 = max(i0, 0);                               // a NaN scale cannot happen; keeps every index in bounds regardless
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
  l0 = 1.0f - l1;
}

__device__ __forceinline__ float2 field_at(const MomentArgs& a, int y, int x) {
#pragma clang fp contract(off)
  const float2* fl = (const float2*)a.flow;
  if (!a.resize) return fl[(int64_t)y * a.fw + x];
  int y0, y1, x0, x1;
  float hy0, hy1, wx0, wx1;
  taps(y, a.scale_y, a.fh, y0, y1, hy0, hy1);
  taps(x, a.scale_x, a.fw, x0, x1, wx0, wx1);
  const float2 v00 = fl[(int64_t)y0 * a.fw + x0], v01 = fl[(int64_t)y0 * a.fw + x1];
  const float2 v10 = fl[(int64_t)y1 * a.fw + x0], v11 = fl[(int64_t)y1 * a.fw + x1];
  float2 r;
  r.x = fmaf(fmaf(v00.x, wx0, v01.x * wx1), hy0, fmaf(v10.x, wx0, v11.x * wx1) * hy1) * a.mul_x;
  r.y = fmaf(fmaf(v00.y, wx0, v01.y * wx1), hy0, fmaf(v10.y, wx0, v11.y * wx1) * hy1) * a.mul_y;
  return r;
}

__global__ void __launch_bounds__(NT) turbulence_moments_kernel(const MomentArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem[];
  const int r = a.radius, k = 2 * r + 1;
  const int aw = TW + 2 * r, ah = TH + 2 * r;
  double* colsum = reinterpret_cast<double*>(smem);                         // [SR][4][aw]
  float2* field = reinterpret_cast<float2*>(colsum + SR * 4 * aw);          // [ah][aw]
  unsigned* hist = reinterpret_cast<unsigned*>(field + ah * aw);            // [BINS1]
  const int tid = threadIdx.x;
  const int ty0 = (blockIdx.x / a.tiles_x) * TH, tx0 = (blockIdx.x % a.tiles_x) * TW;

  for (int i = tid; i < BINS1; i += NT) hist[i] = 0;
  for (int i = tid; i < ah * aw; i += NT) {
    const int ly = i / aw, lx = i - ly * aw;
    field[i] = field_at(a, reflect(ty0 + ly - r, a.h), reflect(tx0 + lx - r, a.w));
  }
  __syncthreads();

  const int oy_l = tid / TW, ox_l = tid - oy_l * TW;      // this thread's output pixel inside a strip
  for (int s = 0; s < TH; s += SR) {
    if (ty0 + s >= a.h) break;                            // uniform: the rest of the tile is below the image
    // columns: k staged rows of one staged column, top to bottom
    for (int i = tid; i < SR * aw; i += NT) {
      const int row = i / aw, c = i - row * aw;
      const float2* p = field + (s + row) * aw + c;
      double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0;
      for (int j = 0; j < k; ++j) {
        const float2 v = lds_f32x2(p + j * aw);
        sx += (double)v.x;
        sy += (double)v.y;
        sxx += (double)(v.x * v.x);                       // the squares are f32 products
        syy += (double)(v.y * v.y);
      }
      double* o = colsum + row * 4 * aw + c;
      o[0] = sx; o[aw] = sy; o[2 * aw] = sxx; o[3 * aw] = syy;
    }
    __syncthreads();
    // rows: k column sums, left to right
    {
      const double* p = colsum + oy_l * 4 * aw + ox_l;
      double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0;
      for (int j = 0; j < k; ++j) {
        sx += vfml_lds_f64(p + j);
        sy += vfml_lds_f64(p + aw + j);
        sxx += vfml_lds_f64(p + 2 * aw + j);
        syy += vfml_lds_f64(p + 3 * aw + j);
      }
      const int y = ty0 + s + oy_l, x = tx0 + ox_l;
      if (y < a.h && x < a.w) {
        const float mx = (float)(sx * a.inv_area), my = (float)(sy * a.inv_area);
        const float mxx = (float)(sxx * a.inv_area), myy = (float)(syy * a.inv_area);
        const float vx = mxx - mx * mx, vy = myy - my * my;
        const float t = root32((vx > 0.0f ? vx : 0.0f) + (vy > 0.0f ? vy : 0.0f));
        a.tv[(int64_t)y * a.w + x] = t;
        atomicAdd(&hist[__float_as_uint(t) >> (32 - BITS1)], 1u);
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < BINS1; i += NT)
    if (const unsigned c = hist[i]) atomicAdd(&a.hist[i], c);
}

// One block of four waves; wave j finds the bin of `hist` row own[j] that holds rank[j], and extends prefix[j] by it.
// STAGE 1 starts from the host's ranks; STAGE 3 ends with the values themselves and numpy's lerp of each pair.
struct SelectArgs {
  const unsigned* hist; SelState* st;
  unsigned rank[4];
  float t[2], one_minus_t[2];       // lerp weights of (lo, hi) and 1 - them, float32
  float* out_lohi;
};

template <int STAGE>
__global__ void __launch_bounds__(256) turbulence_select_kernel(const SelectArgs a) {
#pragma clang fp contract(off)
  constexpr int BINS = STAGE == 1 ? BINS1 : (STAGE == 2 ? BINS2 : BINS3);
  constexpr int BITS = STAGE == 1 ? BITS1 : (STAGE == 2 ? BITS2 : BITS3);
  constexpr int PER = BINS / 64;
  __shared__ unsigned s_prefix[4], s_rank[4];
  const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned rank = STAGE == 1 ? a.rank[j] : a.st->rank[j];
  const unsigned old = STAGE == 1 ? 0u : a.st->prefix[j];
  const unsigned* h = a.hist + (STAGE == 1 ? 0 : (a.st->own[j] & 3u) * BINS) + lane * PER;
  unsigned mine = 0;
  for (int i = 0; i < PER; ++i) mine += h[i];
  unsigned incl = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  if (lane == 0) { s_prefix[j] = old << BITS; s_rank[j] = 0; }     // (a rank beyond the total cannot happen)
  __syncthreads();
  unsigned below = incl - mine;
  if (rank >= below && rank < incl) {
    int i = 0;
    for (; i < PER - 1; ++i) {
      const unsigned c = h[i];
      if (rank < below + c) break;
      below += c;
    }
    s_prefix[j] = (old << BITS) | (unsigned)(lane * PER + i);
    s_rank[j] = rank - below;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 0; q < 4; ++q) {
      int own = q;
      for (int e = q - 1; e >= 0; --e)
        if (s_prefix[e] == s_prefix[q]) own = e;
      a.st->prefix[q] = s_prefix[q];
      a.st->rank[q] = s_rank[q];
      a.st->own[q] = (unsigned)own;
    }
    if constexpr (STAGE == 3) {
      for (int q = 0; q < 2; ++q) {          // numpy _lerp: a + (b - a) t, or b - (b - a)(1 - t) where t >= 0.5
        const float lo = __uint_as_float(s_prefix[2 * q]), hi = __uint_as_float(s_prefix[2 * q + 1]);
        const float d = hi - lo;
        const float v = a.t[q] >= 0.5f ? hi - d * a.one_minus_t[q] : lo + d * a.t[q];
        a.st->lohi[q] = v;
        if (a.out_lohi) a.out_lohi[q] = v;
      }
    }
  }
}

// Histogram of the next bits of the values whose leading bits equal one of the (distinct) prefixes found so far.
template <int STAGE>
__global__ void __launch_bounds__(NT) turbulence_refine_kernel(const float* tv, int64_t n, const SelState* st,
                                                               unsigned* hist_out) {
  constexpr int BINS = STAGE == 2 ? BINS2 : BINS3;
  constexpr int SHIFT = STAGE == 2 ? 32 - BITS1 : 32 - BITS1 - BITS2;     // bits below the prefix
  constexpr int LOW = STAGE == 2 ? BITS3 : 0;                               // bits below this level's digit
  __shared__ unsigned hist[4 * BINS];
  for (int i = threadIdx.x; i < 4 * BINS; i += NT) hist[i] = 0;
  unsigned prefix[4];
  bool owner[4];
  for (int q = 0; q < 4; ++q) {
    prefix[q] = st->prefix[q];
    owner[q] = st->own[q] == (unsigned)q;
  }
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
    const unsigned bits = __float_as_uint(tv[p]);
    const unsigned top = bits >> SHIFT, digit = (bits >> LOW) & (BINS - 1);
    for (int q = 0; q < 4; ++q)
      if (owner[q] && top == prefix[q]) atomicAdd(&hist[q * BINS + digit], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * BINS; i += NT)
    if (const unsigned c = hist[i]) atomicAdd(&hist_out[i], c);
}

__device__ __forceinline__ unsigned jet_index(float t, float lo, float range, bool spread) {
#pragma clang fp contract(off)
  if (!spread) return 0u;
  const float v = div32(t - lo, range);
  const float c = v > 0.0f ? fminf(v, 1.0f) : 0.0f;        // clip(0, 1); NaN -> 0
  return (unsigned)(int)(c * 255.0f);
}

// Four pixels per thread: one 16-byte read of tv, three 4-byte stores of the picture.
__global__ void __launch_bounds__(NT) turbulence_colour_kernel(const float* tv, int64_t n, const SelState* st,
                                                               unsigned char* out_bgr, unsigned char* out_index) {
#pragma clang fp contract(off)
  __shared__ unsigned jet[256];
  jet[threadIdx.x] = JET[threadIdx.x];
  const float lo = st->lohi[0], hi = st->lohi[1];
  const float range = hi - lo;
  const bool spread = range > 1e-6f;
  __syncthreads();
  const int64_t quads = n >> 2;
  for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < quads; q += (int64_t)gridDim.x * NT) {
    const float4 t = reinterpret_cast<const float4*>(tv)[q];
    const unsigned i0 = jet_index(t.x, lo, range, spread), i1 = jet_index(t.y, lo, range, spread);
    const unsigned i2 = jet_index(t.z, lo, range, spread), i3 = jet_index(t.w, lo, range, spread);
    const unsigned c0 = jet[i0], c1 = jet[i1], c2 = jet[i2], c3 = jet[i3];     // 0x00RRGGBB: bytes B, G, R in memory
    unsigned* o = reinterpret_cast<unsigned*>(out_bgr) + 3 * q;
    o[0] = c0 | (c1 << 24);
    o[1] = (c1 >> 8) | (c2 << 16);
    o[2] = (c2 >> 16) | (c3 << 8);
    if (out_index) reinterpret_cast<unsigned*>(out_index)[q] = i0 | (i1 << 8) | (i2 << 16) | (i3 << 24);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) {
    const int64_t p = (quads << 2) + threadIdx.x;
    const unsigned i = jet_index(tv[p], lo, range, spread), c = jet[i];
    out_bgr[3 * p] = (unsigned char)c;
    out_bgr[3 * p + 1] = (unsigned char)(c >> 8);
    out_bgr[3 * p + 2] = (unsigned char)(c >> 16);
    if (out_index) out_index[p] = (unsigned char)i;
  }
}

inline int stream_blocks(int64_t items) {
  const int64_t g = (items + NT - 1) / NT;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

inline size_t moments_lds(int radius) {
  const size_t aw = TW + 2 * radius, ah = TH + 2 * radius;
  return sizeof(double) * SR * 4 * aw + sizeof(float2) * ah * aw + sizeof(unsigned) * BINS1;
}

// numpy's percentile (method 'linear') on a float32 array of n values, as numpy 2 evaluates it: the quantile, the
// virtual index and the weight are all float32
inline void percentile_plan(int64_t n, float percent, unsigned& prev, unsigned& next, float& t) {
#pragma clang fp contract(off)
  const float q = percent / 100.0f;
  const float vi = (float)(n - 1) * q;
  float p = floorf(vi), nx = p + 1.0f;
  if (vi >= (float)(n - 1)) p = nx = -1.0f;
  if (vi < 0.0f) p = nx = 0.0f;
  t = vi - p;
  int64_t ip = (int64_t)p, in = (int64_t)nx;
  if (ip < 0) ip += n;
  if (in < 0) in += n;
  prev = (unsigned)(ip < 0 ? 0 : (ip > n - 1 ? n - 1 : ip));
  next = (unsigned)(in < 0 ? 0 : (in > n - 1 ? n - 1 : in));
}

}  // namespace

extern "C" size_t vfml_flow_turbulence_workspace_bytes(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return layout((int64_t)h * w).total;
}

extern "C" int vfml_flow_turbulence_map(const float* flow, int fh, int fw, int h, int w, int ksize, void* workspace,
                                        unsigned char* out_bgr, unsigned char* out_index, float* out_tv,
                                        float* out_lohi, void* stream) {
#pragma clang fp contract(off)
  VFML_REQUIRE(ksize >= 1 && ksize <= 2 * MAX_RADIUS + 1 && (ksize & 1) == 1,
               "vfml_flow_turbulence_map: ksize %d is not an odd number in 1..%d", ksize, 2 * MAX_RADIUS + 1);
  VFML_REQUIRE(flow && workspace && out_bgr && h > 0 && w > 0 && fh > 0 && fw > 0, "vfml_flow_turbulence_map: bad argument");
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(flow) & 7u) == 0, "vfml_flow_turbulence_map: flow must be 8-byte aligned");
  VFML_REQUIRE(h <= (1 << 24) && w <= (1 << 24) && (int64_t)h * w < (1ll << 31),
               "vfml_flow_turbulence_map: picture too large (side above 2^24 or 2^31 pixels)");
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "vfml_flow_turbulence_map: workspace must be 256-byte aligned");
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(out_bgr) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_index) & 3u) == 0 &&
               vfml_aligned16(out_tv) && (reinterpret_cast<uintptr_t>(out_lohi) & 3u) == 0,
               "vfml_flow_turbulence_map: out_bgr / out_index / out_lohi must be 4-byte, out_tv 16-byte aligned");
  const int64_t n = (int64_t)h * w;
  const Workspace ws = layout(n);
  unsigned char* base = static_cast<unsigned char*>(workspace);
  unsigned* hist1 = reinterpret_cast<unsigned*>(base + ws.hist1);
  unsigned* hist2 = reinterpret_cast<unsigned*>(base + ws.hist2);
  unsigned* hist3 = reinterpret_cast<unsigned*>(base + ws.hist3);
  SelState* st = reinterpret_cast<SelState*>(base + ws.state);
  float* tv = out_tv ? out_tv : reinterpret_cast<float*>(base + ws.tv);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);

  MomentArgs a;
  a.flow = flow; a.tv = tv; a.hist = hist1;
  a.h = h; a.w = w; a.fh = fh; a.fw = fw; a.radius = ksize / 2;
  a.resize = (fh != h || fw != w) ? 1 : 0;
  a.tiles_x = (w + TW - 1) / TW;
  a.scale_y = (float)fh / (float)h;
  a.scale_x = (float)fw / (float)w;
  a.mul_x = (float)((double)w / (double)fw);
  a.mul_y = (float)((double)h / (double)fh);
  a.inv_area = 1.0 / ((double)ksize * (double)ksize);
  const int64_t tiles = (int64_t)a.tiles_x * ((h + TH - 1) / TH);
  VFML_REQUIRE(tiles < (1ll << 31), "vfml_flow_turbulence_map: too many tiles");

  SelectArgs sa;
  sa.hist = hist1; sa.st = st; sa.out_lohi = out_lohi;
  percentile_plan(n, 5.0f, sa.rank[0], sa.rank[1], sa.t[0]);
  percentile_plan(n, 95.0f, sa.rank[2], sa.rank[3], sa.t[1]);
  sa.one_minus_t[0] = 1.0f - sa.t[0];
  sa.one_minus_t[1] = 1.0f - sa.t[1];

  const size_t lds = moments_lds(a.radius);
  if (const int rc = vfml_lds_cap(reinterpret_cast<const void*>(&turbulence_moments_kernel), (int)moments_lds(MAX_RADIUS),
                                  "vfml_flow_turbulence_map")) return rc;
  const hipError_t e = hipMemsetAsync(base + ws.hist1, 0, ws.state - ws.hist1, s);
  if (e != hipSuccess) {
    vfml_set_error("vfml_flow_turbulence_map: hipMemsetAsync: %s", hipGetErrorString(e));
    return 2;
  }
  const dim3 one(1), block(NT), stream_grid(stream_blocks(n));
  hipLaunchKernelGGL(turbulence_moments_kernel, dim3((unsigned)tiles), block, lds, s, a);
  hipLaunchKernelGGL(turbulence_select_kernel<1>, one, block, 0, s, sa);
  hipLaunchKernelGGL(turbulence_refine_kernel<2>, stream_grid, block, 0, s, (const float*)tv, n, (const SelState*)st, hist2);
  sa.hist = hist2;
  hipLaunchKernelGGL(turbulence_select_kernel<2>, one, block, 0, s, sa);
  hipLaunchKernelGGL(turbulence_refine_kernel<3>, stream_grid, block, 0, s, (const float*)tv, n, (const SelState*)st, hist3);
  sa.hist = hist3;
  hipLaunchKernelGGL(turbulence_select_kernel<3>, one, block, 0, s, sa);
  hipLaunchKernelGGL(turbulence_colour_kernel, dim3(stream_blocks((n + 3) / 4)), block, 0, s, (const float*)tv, n,
                     (const SelState*)st, out_bgr, out_index);
  return vfml_check_launch("vfml_flow_turbulence_map");
}
