// Batch flow-cache correction (reference correction_worker.py: worker_process :221-341): for every "bad" pixel of a
// frame's quality map, re-estimate its vector with a phase correlation of two 50x50 grey regions seeded from a cached
// LOD, fall back to an 11x11 TM_CCOEFF_NORMED template match plus a spiral search, and keep the better result when it
// beats the pixel's current match.  DESIGN.md section 8 defines the OpenCV primitives and every rounding step.
//
// One frame per call, all on the caller's stream, no host synchronisation:
//   quality map -> bad-pixel list in raster order (block counts, one-block scan, compaction: no atomics)
//   -> coarse kernel (one workgroup per bad pixel, persistent grid; regions and spectra in LDS as f64)
//   -> fine kernel (one workgroup per bad pixel; also applies the accept rule and writes the corrected vector)
//   -> quality map of the corrected flow -> its bad-pixel count.
// Every bad pixel is independent: it reads the ORIGINAL flow and LOD and writes only its own cell of the copy.
//
// All arithmetic is f64 without contraction unless a rule says otherwise; the float32 steps are the ones numpy >= 2
// (NEP 50) takes in the reference, where a float32 flow value meets a Python float.  LDS f64 values are read through
// vfml_lds_f64 (see vfml_common.h).
#include "vfml_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int N = 50;                 // phase-correlation region side (2 * 25)
constexpr int NN = N * N;
constexpr int TS = 11;                // template side (int(2 * 5.5))
constexpr int TN = TS * TS;
constexpr int SR = 50;                // search-area rows (2 * 25)
constexpr int CT = 512;               // coarse workgroup
constexpr int FT = 256;               // fine workgroup
constexpr int ST = 256;               // scan workgroup
constexpr int SPT = 4;                // pixels per scan thread
constexpr int CHUNK = ST * SPT;
constexpr double EPS52 = 2.220446049250313080847e-16;   // 2^-52

// LDS map of the coarse kernel (doubles)
constexpr int L_TW = 0;               // cos[50], sin[50]
constexpr int L_XAR = 100, L_XAI = L_XAR + NN, L_XBR = L_XAI + NN, L_XBI = L_XBR + NN;   // row-pass spectra
constexpr int L_CR = L_XBI + NN, L_CI = L_CR + NN;                                       // cross-power
constexpr int L_GA = L_CR, L_GB = L_CI;          // grey regions (dead before the cross-power is written)
constexpr int L_YR = L_XAR, L_YI = L_XAI;        // inverse row pass
constexpr int L_R = L_XBR;                       // correlation surface
constexpr int L_RV = L_XBI;                      // argmax reduction values
constexpr int L_TOTAL = L_CI + NN;

struct CorrState {            // per bad pixel, coarse kernel -> fine kernel (64 B)
  double orig_sim, csim, tx, ty, shx, shy;
  float lvx, lvy, cfx, cfy;
};

struct CorrArgs {
  const unsigned char* f1; const unsigned char* f2; const float* flow; const float* lod; const double* tw;
  float* out; double* rec; int64_t rec_cap;
  const int* list; const int* nbad; CorrState* st;
  int h, w, lh, lw;
  double lsx, lsy;            // lw / w, lh / h
  double good, fine_thr;
};

__device__ __forceinline__ double lds(const double* p) { return vfml_lds_f64(p); }
// an int read from LDS whose first reader is a 32-bit move: the template products would otherwise take it straight into
// v_mad_u64_u32 (a 64-bit-operand op; vfml_common.h, vfml_lds_f64)
__device__ __forceinline__ int lds_i32(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  int v = *p, r;
  asm("v_mov_b32 %0, %1" : "=v"(r) : "v"(v));
  return r;
#else
  return *p;
#endif
}

// colour similarity of two u8 RGB pixels (reference calculate_pixel_quality :9-27)
__device__ double similarity(const unsigned char* p, const unsigned char* q) {
  const double rgb_max = 0x1.b9ac46d6ff45ep+8;   // sqrt(195075), correctly rounded
  const double a0 = p[0], a1 = p[1], a2 = p[2], b0 = q[0], b1 = q[1], b2 = q[2];
  const double d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
  const double rgb = 1.0 - sqrt((d0 * d0 + d1 * d1) + d2 * d2) / rgb_max;
  const double mad = 1.0 - ((fabs(d0) + fabs(d1)) + fabs(d2)) / 3.0 / 255.0;
  const double na = sqrt((a0 * a0 + a1 * a1) + a2 * a2), nb = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
  double cs;
  if (na > 1e-6 && nb > 1e-6) cs = (((a0 * b0 + a1 * b1) + a2 * b2) / (na * nb) + 1.0) / 2.0;
  else cs = 1.0 - fabs(na - nb) / rgb_max;
  return (rgb + mad + cs) / 3.0;
}

// Python int() of a float64, clamped to +-2^30 (wider values act the same in every bound they feed); NaN -> 0
__device__ __forceinline__ int pyint(double v) {
  if (!(v == v)) return 0;
  const double t = trunc(v);
  return (int)fmin(fmax(t, -1073741824.0), 1073741824.0);
}
// range(n)[start:stop] for start >= 0 -> first index and length
__device__ __forceinline__ void pyslice(int start, int stop, int n, int& first, int& len) {
  if (stop < 0) stop = max(0, n + stop);
  start = min(start, n);
  stop = min(stop, n);
  first = start;
  len = max(0, stop - start);
}
__device__ __forceinline__ double grey(const unsigned char* p) {
  return (double)(((int)p[0] * 4899 + (int)p[1] * 9617 + (int)p[2] * 1868 + 8192) >> 14);
}
// float32 quotient, correctly rounded (through the float64 one)
__device__ __forceinline__ float div32(float x, float y) { return (float)((double)x / (double)y); }

// ---- bad-pixel list ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int block_sum(int v, int* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = ST / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const int t = red[0];
  __syncthreads();
  return t;
}

__global__ void __launch_bounds__(ST) bad_count_kernel(const unsigned char* map, int64_t n, int* blk) {
  __shared__ int red[ST];
  const int64_t p0 = (int64_t)blockIdx.x * CHUNK + (int64_t)threadIdx.x * SPT;
  int c = 0;
  for (int k = 0; k < SPT; ++k) c += (p0 + k < n && map[3 * (p0 + k)] > 0) ? 1 : 0;
  const int t = block_sum(c, red);
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}

// one workgroup: exclusive offsets of the block counts, total into *total
__global__ void __launch_bounds__(1024) bad_scan_kernel(const int* blk, int nb, int* off, int* total) {
  __shared__ int s[1024];
  int carry = 0;
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + (int)threadIdx.x;
    const int v = i < nb ? blk[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int add = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < nb) off[i] = carry + s[threadIdx.x] - v;
    carry += s[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ void __launch_bounds__(ST) bad_compact_kernel(const unsigned char* map, int64_t n, const int* off, int* list) {
  __shared__ int s[ST];
  const int64_t p0 = (int64_t)blockIdx.x * CHUNK + (int64_t)threadIdx.x * SPT;
  bool f[SPT];
  int c = 0;
  for (int k = 0; k < SPT; ++k) {
    f[k] = p0 + k < n && map[3 * (p0 + k)] > 0;
    c += f[k] ? 1 : 0;
  }
  s[threadIdx.x] = c;
  __syncthreads();
  for (int d = 1; d < ST; d <<= 1) {
    const int add = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  int o = off[blockIdx.x] + s[threadIdx.x] - c;
  for (int k = 0; k < SPT; ++k)
    if (f[k]) list[o++] = (int)(p0 + k);
}

// ---- coarse step: original similarity, LOD vector, phase correlation ------------------------------------------------
// one length-50 DFT term sum over an LDS operand: out = sum_j x[j * stride] * w[(j * k) mod 50] (ascending j);
// conj selects the inverse twiddle (cos, +sin) instead of (cos, -sin)
__device__ __forceinline__ void dft_sum(const double* S, int re, int im, int stride, int k, bool conj, bool real_in,
                                        double& out_re, double& out_im) {
  double ar = 0.0, ai = 0.0;
  int m = 0;
  for (int j = 0; j < N; ++j) {
    const double a = lds(S + re + j * stride), b = real_in ? 0.0 : lds(S + im + j * stride);
    const double c = lds(S + L_TW + m), sn = lds(S + L_TW + N + m);
    const double d = conj ? sn : -sn;
    ar = ar + (a * c - b * d);
    ai = ai + (a * d + b * c);
    m += k;
    if (m >= N) m -= N;
  }
  out_re = ar;
  out_im = ai;
}

__global__ void __launch_bounds__(CT) correct_coarse_kernel(const CorrArgs a) {
  __shared__ double S[L_TOTAL];
  __shared__ int RI[CT];
  const int tid = threadIdx.x;
  const int nbad = *a.nbad;
  for (int t = tid; t < 2 * N; t += CT) S[L_TW + t] = a.tw[t];
  for (int i = blockIdx.x; i < nbad; i += gridDim.x) {
    const int p = a.list[i];
    const int y = p / a.w, x = p - y * a.w;
    // LOD texel and vector (float32 value / float32(scale), as numpy >= 2 divides a float32 by a Python float)
    const int lx = max(0, min((int)((double)x * a.lsx), a.lw - 1)), ly = max(0, min((int)((double)y * a.lsy), a.lh - 1));
    const float2 lv = ((const float2*)a.lod)[(int64_t)ly * a.lw + lx];
    const float lvx = div32(lv.x, (float)a.lsx), lvy = div32(lv.y, (float)a.lsy);
    // regions: frame1 around the pixel, frame2 around the LOD target; bottom/right zero padding to 50
    int r1x, r1nx, r1y, r1ny, r2x, r2nx, r2y, r2ny;
    pyslice(max(0, x - 25), min(a.w, x + 25), a.w, r1x, r1nx);
    pyslice(max(0, y - 25), min(a.h, y + 25), a.h, r1y, r1ny);
    const double cx = (double)x - (double)lvx, cy = (double)y - (double)lvy;
    pyslice(max(0, pyint(cx - 25.0)), min(a.w, pyint(cx + 25.0)), a.w, r2x, r2nx);
    pyslice(max(0, pyint(cy - 25.0)), min(a.h, pyint(cy + 25.0)), a.h, r2y, r2ny);
    __syncthreads();                                  // previous pixel done with the LDS
    for (int o = tid; o < 2 * NN; o += CT) {
      const int img = o >= NN, q = o - img * NN, r = q / N, c = q - r * N;
      double g = 0.0;
      if (!img) {
        if (r < r1ny && c < r1nx) g = grey(a.f1 + 3 * ((int64_t)(r1y + r) * a.w + (r1x + c)));
      } else {
        if (r < r2ny && c < r2nx) g = grey(a.f2 + 3 * ((int64_t)(r2y + r) * a.w + (r2x + c)));
      }
      S[(img ? L_GB : L_GA) + q] = g;
    }
    __syncthreads();
    // forward row pass of both regions
    for (int o = tid; o < 2 * NN; o += CT) {
      const int img = o >= NN, q = o - img * NN, r = q / N, k = q - r * N;
      double re, im;
      dft_sum(S, (img ? L_GB : L_GA) + r * N, 0, 1, k, false, true, re, im);
      S[(img ? L_XBR : L_XAR) + q] = re;
      S[(img ? L_XBI : L_XAI) + q] = im;
    }
    __syncthreads();
    // forward column pass of both, then the normalised cross-power spectrum Fa conj(Fb)
    for (int q = tid; q < NN; q += CT) {
      const int k1 = q / N, k2 = q - k1 * N;
      double far, fai, fbr, fbi;
      dft_sum(S, L_XAR + k2, L_XAI + k2, N, k1, false, false, far, fai);
      dft_sum(S, L_XBR + k2, L_XBI + k2, N, k1, false, false, fbr, fbi);
      const double nbi = -fbi;
      const double pr = far * fbr - fai * nbi, pi = far * nbi + fai * fbr;
      const double mag = sqrt(pr * pr + pi * pi);
      const double den = mag * mag + EPS52;
      S[L_CR + q] = pr * mag / den;
      S[L_CI + q] = pi * mag / den;
    }
    __syncthreads();
    // inverse row pass
    for (int q = tid; q < NN; q += CT) {
      const int r = q / N, k = q - r * N;
      double re, im;
      dft_sum(S, L_CR + r * N, L_CI + r * N, 1, k, true, false, re, im);
      S[L_YR + q] = re;
      S[L_YI + q] = im;
    }
    __syncthreads();
    // inverse column pass, real part
    for (int q = tid; q < NN; q += CT) {
      const int k1 = q / N, k2 = q - k1 * N;
      double re, im;
      dft_sum(S, L_YR + k2, L_YI + k2, N, k1, true, false, re, im);
      S[L_R + q] = re;
    }
    __syncthreads();
    // fftShift, then the first maximum in raster order
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int q = tid; q < NN; q += CT) {
      const int sy = q / N, sx = q - sy * N;
      const double v = lds(S + L_R + ((sy + N / 2) % N) * N + (sx + N / 2) % N);
      if (v > bv) { bv = v; bi = q; }
    }
    S[L_RV + tid] = bv;
    RI[tid] = bi;
    __syncthreads();
    for (int s = CT / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const double v0 = lds(S + L_RV + tid), v1 = lds(S + L_RV + tid + s);
        const int i0 = RI[tid], i1 = RI[tid + s];
        if (v1 > v0 || (v1 == v0 && i1 < i0)) { S[L_RV + tid] = v1; RI[tid] = i1; }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int peak = RI[0], py = peak / N, px = peak - py * N;
      double sxv = 0.0, syv = 0.0, sum = 0.0;
      for (int yy = max(0, py - 2); yy <= min(N - 1, py + 2); ++yy)
        for (int xx = max(0, px - 2); xx <= min(N - 1, px + 2); ++xx) {
          const double v = lds(S + L_R + ((yy + N / 2) % N) * N + (xx + N / 2) % N);
          sxv = sxv + (double)xx * v;
          syv = syv + (double)yy * v;
          sum = sum + v;
        }
      sum = sum + EPS52;
      const double shx = (double)N / 2.0 - sxv / sum, shy = (double)N / 2.0 - syv / sum;
      // coarse vector: float32 LOD vector minus float32(shift); target in float64
      const float cfx = lvx - (float)shx, cfy = lvy - (float)shy;
      const double tx = (double)x - (double)cfx, ty = (double)y - (double)cfy;
      const unsigned char* src = a.f1 + 3 * (int64_t)p;
      double csim = 0.0;
      if (tx >= 0.0 && tx < (double)a.w && ty >= 0.0 && ty < (double)a.h)
        csim = similarity(src, a.f2 + 3 * ((int64_t)(int)ty * a.w + (int)tx));
      // the pixel's current match: its own vector, target rounded half to even
      const float2 fv = ((const float2*)a.flow)[p];
      const double ox = rint((double)x - (double)fv.x), oy = rint((double)y - (double)fv.y);
      double orig = 0.0;
      if (ox >= 0.0 && ox < (double)a.w && oy >= 0.0 && oy < (double)a.h)
        orig = similarity(src, a.f2 + 3 * ((int64_t)(int)oy * a.w + (int)ox));
      CorrState st;
      st.orig_sim = orig; st.csim = csim; st.tx = tx; st.ty = ty; st.shx = shx; st.shy = shy;
      st.lvx = lvx; st.lvy = lvy; st.cfx = cfx; st.cfy = cfy;
      a.st[i] = st;
    }
  }
}

// ---- fine step (template match + spiral), choice, accept, write -------------------------------------------------------
__global__ void __launch_bounds__(FT) correct_fine_kernel(const CorrArgs a) {
  __shared__ int T[TN * 3];
  __shared__ float RV[FT];
  __shared__ int RI[FT];
  const int tid = threadIdx.x;
  const int nbad = *a.nbad;
  for (int i = blockIdx.x; i < nbad; i += gridDim.x) {
    const int p = a.list[i];
    const int y = p / a.w, x = p - y * a.w;
    const CorrState st = a.st[i];
    const unsigned char* src = a.f1 + 3 * (int64_t)p;
    const bool attempt = st.csim < a.fine_thr;
    bool valid = false;
    double fx = 0.0, fy = 0.0, fsim = 0.0;
    // geometry (uniform over the workgroup)
    int tx0, tnx, ty0, tny, sx0, snx, sy0, sny;
    pyslice(max(0, pyint((double)x - 5.5)), min(a.w, pyint((double)x + 5.5)), a.w, tx0, tnx);
    pyslice(max(0, pyint((double)y - 5.5)), min(a.h, pyint((double)y + 5.5)), a.h, ty0, tny);
    const int sx1 = max(0, pyint(st.tx - 25.0)), sy1 = max(0, pyint(st.ty - 25.0));
    pyslice(sx1, min(a.w, pyint(st.tx + 25.0)), a.w, sx0, snx);
    pyslice(sy1, min(a.h, pyint(st.ty + 25.0)), a.h, sy0, sny);
    const int cols = max(snx, SR);
    // rows only, as the reference checks: the template is always 11 rows, the area 50 unless a slice is longer
    if (attempt && max(tny, TS) == TS && max(sny, SR) == SR) {
      __syncthreads();                                 // previous pixel done with the LDS
      for (int t = tid; t < TN * 3; t += FT) {
        const int c = t % 3, q = t / 3, r = q / TS, cc = q - r * TS;
        T[t] = (r < tny && cc < tnx) ? (int)a.f1[3 * ((int64_t)(ty0 + r) * a.w + (tx0 + cc)) + c] : 0;
      }
      __syncthreads();
      int st_[3] = {0, 0, 0}, st2[3] = {0, 0, 0};
      for (int t = 0; t < TN; ++t)
        for (int c = 0; c < 3; ++c) {
          const int v = lds_i32(T + 3 * t + c);
          st_[c] += v;
          st2[c] += v * v;
        }
      int64_t tv = 0;
      for (int c = 0; c < 3; ++c) tv += (int64_t)(TN * st2[c] - st_[c] * st_[c]);
      const int ow = cols - TS + 1, npos = (SR - TS + 1) * ow;
      float bv = -2.0f;
      int bi = 0x7fffffff;
      for (int q = tid; q < npos; q += FT) {
        const int py = q / ow, px = q - py * ow;
        int sti[3] = {0, 0, 0}, si[3] = {0, 0, 0}, si2[3] = {0, 0, 0};
        for (int r = 0; r < TS; ++r) {
          const int rr = py + r;
          if (rr >= sny) break;                           // zero padding below
          const unsigned char* row = a.f2 + 3 * ((int64_t)(sy0 + rr) * a.w + sx0);
          const int jn = min(TS, snx - px);               // zero padding at the right
          for (int j = 0; j < jn; ++j) {
            const unsigned char* pp = row + 3 * (px + j);
            const int* tp = T + 3 * (r * TS + j);
            for (int c = 0; c < 3; ++c) {
              const int v = pp[c];
              sti[c] += lds_i32(tp + c) * v;
              si[c] += v;
              si2[c] += v * v;
            }
          }
        }
        int64_t num = 0, wv = 0;
        for (int c = 0; c < 3; ++c) {
          num += (int64_t)(TN * sti[c] - st_[c] * si[c]);
          wv += (int64_t)(TN * si2[c] - si[c] * si[c]);
        }
        float rv;
        if (tv == 0) rv = 1.0f;
        else if (wv == 0) rv = 0.0f;
        else rv = (float)fmin(fmax((double)num / (sqrt((double)tv) * sqrt((double)wv)), -1.0), 1.0);
        if (rv > bv) { bv = rv; bi = q; }
      }
      RV[tid] = bv;
      RI[tid] = bi;
      __syncthreads();
      for (int s = FT / 2; s > 0; s >>= 1) {
        if (tid < s) {
          const float v0 = RV[tid], v1 = RV[tid + s];
          const int i0 = RI[tid], i1 = RI[tid + s];
          if (v1 > v0 || (v1 == v0 && i1 < i0)) { RV[tid] = v1; RI[tid] = i1; }
        }
        __syncthreads();
      }
      if (tid == 0) {
        const int loc = RI[0], ly = loc / ow, lx = loc - ly * ow;
        const double pcx = (double)(sx1 + lx) + 5.5, pcy = (double)(sy1 + ly) + 5.5;
        if (pcx >= 0.0 && pcx < (double)a.w && pcy >= 0.0 && pcy < (double)a.h) {
          valid = true;
          double bx = pcx, by = pcy;
          fsim = similarity(src, a.f2 + 3 * ((int64_t)(int)pcy * a.w + (int)pcx));
          if (!(fsim > a.good)) {                         // spiral outwards, first in-frame match above the bar
            int ox = 0, oy = 0, dx = 0, dy = -1;
            for (int it = 0; it < TS * TS; ++it) {
              if (-5.5 < ox && ox <= 5.5 && -5.5 < oy && oy <= 5.5) {
                const double qx = pcx + ox, qy = pcy + oy;
                if (qx >= 0.0 && qx < (double)a.w && qy >= 0.0 && qy < (double)a.h) {
                  const double s = similarity(src, a.f2 + 3 * ((int64_t)(int)qy * a.w + (int)qx));
                  if (s > a.good) { bx = qx; by = qy; fsim = s; break; }
                }
              }
              if (ox == oy || (ox < 0 && ox == -oy) || (ox > 0 && ox == 1 - oy)) { const int t = dx; dx = -dy; dy = t; }
              ox += dx;
              oy += dy;
            }
          }
          fx = (double)x - bx;
          fy = (double)y - by;
        }
      }
    }
    if (tid == 0) {
      double vx = (double)st.cfx, vy = (double)st.cfy, sim = st.csim;
      if (valid && fsim > st.csim) { vx = fx; vy = fy; sim = fsim; }
      const bool accept = sim > a.good || sim > st.orig_sim;
      if (accept) ((float2*)a.out)[p] = make_float2((float)vx, (float)vy);
      if (a.rec && i < a.rec_cap) {
        double* r = a.rec + (int64_t)i * VFML_CORRECT_RECORD;
        r[0] = (double)p; r[1] = st.orig_sim; r[2] = (double)st.lvx; r[3] = (double)st.lvy;
        r[4] = st.shx; r[5] = st.shy; r[6] = (double)st.cfx; r[7] = (double)st.cfy; r[8] = st.csim;
        r[9] = attempt ? 1.0 : 0.0; r[10] = valid ? 1.0 : 0.0;
        r[11] = valid ? fx : 0.0; r[12] = valid ? fy : 0.0; r[13] = valid ? fsim : 0.0;
        r[14] = accept ? 1.0 : 0.0; r[15] = 0.0;
      }
    }
  }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
  size_t map, blk, off, list, st, total;
};
inline Layout layout(int h, int w) {
  const int64_t n = (int64_t)h * w, nb = (n + CHUNK - 1) / CHUNK;
  Layout l;
  l.map = 0;
  l.blk = align256((size_t)(3 * n));
  l.off = l.blk + align256((size_t)nb * 4);
  l.list = l.off + align256((size_t)nb * 4);
  l.st = l.list + align256((size_t)n * 4);
  l.total = l.st + align256((size_t)n * sizeof(CorrState));
  return l;
}

int count_bad(const unsigned char* map, int64_t n, int* blk, int* off, int* total, int* list, hipStream_t s) {
  const int nb = (int)((n + CHUNK - 1) / CHUNK);
  hipLaunchKernelGGL(bad_count_kernel, dim3(nb), dim3(ST), 0, s, map, n, blk);
  hipLaunchKernelGGL(bad_scan_kernel, dim3(1), dim3(1024), 0, s, blk, nb, off, total);
  if (list) hipLaunchKernelGGL(bad_compact_kernel, dim3(nb), dim3(ST), 0, s, map, n, off, list);
  return vfml_check_launch("vfml_flow_correct (bad-pixel list)");
}

}  // namespace

extern "C" size_t vfml_flow_correct_workspace_bytes(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return layout(h, w).total;
}

extern "C" int vfml_flow_correct(const unsigned char* frame1, const unsigned char* frame2, const float* flow,
                                 const float* lod, int lh, int lw, int h, int w, const double* twiddles,
                                 double good_threshold, double fine_threshold, double region_radius,
                                 double template_radius, double search_radius, float* out_flow, int* counts,
                                 double* records, int64_t record_capacity, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  VFML_REQUIRE(frame1 && frame2 && flow && lod && twiddles && out_flow && counts && workspace,
               "vfml_flow_correct: null argument");
  VFML_REQUIRE(h > 0 && w > 0 && lh > 0 && lw > 0, "vfml_flow_correct: bad size %dx%d (LOD %dx%d)", h, w, lh, lw);
  VFML_REQUIRE((int64_t)h * w <= (1 << 30), "vfml_flow_correct: frame above 2^30 pixels");
  VFML_REQUIRE(region_radius == 25.0 && template_radius == 5.5 && search_radius == 25.0,
               "vfml_flow_correct: unsupported radii (region %g, template %g, search %g): only 25 / 5.5 / 25",
               region_radius, template_radius, search_radius);
  VFML_REQUIRE(((reinterpret_cast<uintptr_t>(flow) | reinterpret_cast<uintptr_t>(lod) |
                 reinterpret_cast<uintptr_t>(out_flow)) & 7u) == 0, "vfml_flow_correct: flow, LOD and output must be 8-byte aligned");
  VFML_REQUIRE(out_flow != flow && out_flow != lod, "vfml_flow_correct: the output may not alias the flow or the LOD");
  VFML_REQUIRE(record_capacity >= 0 && (records || record_capacity == 0), "vfml_flow_correct: bad record buffer");
  const Layout L = layout(h, w);
  VFML_REQUIRE(workspace_bytes >= L.total, "vfml_flow_correct: workspace %zu B, needs %zu", workspace_bytes, L.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  unsigned char* map = reinterpret_cast<unsigned char*>(ws + L.map);
  int* blk = reinterpret_cast<int*>(ws + L.blk);
  int* off = reinterpret_cast<int*>(ws + L.off);
  int* list = reinterpret_cast<int*>(ws + L.list);
  const int64_t n = (int64_t)h * w;
  const float thr = (float)good_threshold;
  if (vfml_flow_quality_map(frame1, frame2, flow, h, w, h, w, thr, map, stream)) return 1;
  if (count_bad(map, n, blk, off, counts, list, s)) return 2;
  if (hipMemcpyAsync(out_flow, flow, (size_t)n * 8, hipMemcpyDeviceToDevice, s) != hipSuccess) {
    vfml_set_error("vfml_flow_correct: flow copy failed");
    return 2;
  }
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  CorrArgs a;
  a.f1 = frame1; a.f2 = frame2; a.flow = flow; a.lod = lod; a.tw = twiddles;
  a.out = out_flow; a.rec = records; a.rec_cap = record_capacity;
  a.list = list; a.nbad = counts; a.st = reinterpret_cast<CorrState*>(ws + L.st);
  a.h = h; a.w = w; a.lh = lh; a.lw = lw;
  a.lsx = (double)lw / (double)w;
  a.lsy = (double)lh / (double)h;
  a.good = good_threshold;
  a.fine_thr = fine_threshold;
  hipLaunchKernelGGL(correct_coarse_kernel, dim3(cus), dim3(CT), 0, s, a);
  if (vfml_check_launch("vfml_flow_correct (coarse)")) return 2;
  hipLaunchKernelGGL(correct_fine_kernel, dim3(4 * cus), dim3(FT), 0, s, a);
  if (vfml_check_launch("vfml_flow_correct (fine)")) return 2;
  if (vfml_flow_quality_map(frame1, frame2, out_flow, h, w, h, w, thr, map, stream)) return 1;
  return count_bad(map, n, blk, off, counts + 1, nullptr, s);
}
