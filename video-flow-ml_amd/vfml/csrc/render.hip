// Render stage of flow_processor's output video: the two colour-wheel
// flow encoders and the frame composer.  Both are elementwise and HBM-bound; neither is fused with the TAA step or the
// other encoders (the render rate is set by the host's JPEG encoder / disk and the copy back, not by these kernels).
//
// vfml_flow_colorize: a grid-stride max reduction of the per-pixel magnitude into a u32 cell of `workspace` (atomic max
// on the bit pattern of a non-negative float: exact, order-free), then one thread per pixel reads the cell.  No host
// synchronisation.  Every float32 step is rounded separately (contract off), in the order numpy / the torchvision
// definition takes them; atan2 is the float64 one rounded to float32 (host and stand-in do the same).
//
// vfml_compose_frame: one thread per output dword of a row; each byte finds its tile, pixel and channel, so the buffer
// handed to the AVI writer is the chunk payload itself (channel order, row order, padded row stride).
//
// vfml_flow_decode / vfml_flow_diff_overlay (the --flow-input comparison): one thread per pixel.  The decoder takes the
// host decoders' float32 steps in their order; the overlay classifies |a - b| against the float32 thresholds and decides
// the legend's squares from the pixel's coordinates in the same pass.
#include "vfml_common.h"

namespace {

constexpr float kPi32 = 3.14159265358979323846f;          // float32(np.pi) / float32(torch.pi)
constexpr float kTwoPi32 = 6.28318530717958647692f;       // float32(2 * np.pi)
constexpr float kFltEps = 1.1920928955078125e-07f;        // torch.finfo(float32).eps

inline int blocks_for(int64_t items, int block) {
  int64_t g = (items + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

// float -> uint8 as numpy's astype(np.uint8) does on x86-64: truncate to int32, keep the low byte; NaN, +-inf and values
// outside int32 give 0
__device__ __forceinline__ unsigned char u8_trunc(float x) {
  return (x > -2147483648.0f && x < 2147483648.0f) ? (unsigned char)(int)x : (unsigned char)0;
}
__device__ __forceinline__ unsigned char u8_trunc64(double x) {
  return (x > -2147483648.0 && x < 2147483648.0) ? (unsigned char)(int)x : (unsigned char)0;
}
__device__ __forceinline__ float root32(float x) { return (float)sqrt((double)x); }     // correctly rounded
__device__ __forceinline__ float div32(float x, float y) { return (float)((double)x / (double)y); }
__device__ __forceinline__ float atan2_32(float y, float x) { return (float)atan2((double)y, (double)x); }
// np.nan_to_num(nan=0, posinf=1, neginf=-1)
__device__ __forceinline__ float hsv_clean(float v) {
  if (v != v) return 0.0f;
  if (v == __builtin_huge_valf()) return 1.0f;
  if (v == -__builtin_huge_valf()) return -1.0f;
  return v;
}

// per-pixel magnitude whose frame maximum normalises the colour: HSV after nan_to_num, WHEEL on the raw field
template <int MODE>
__device__ __forceinline__ float magnitude(float2 f) {
#pragma clang fp contract(off)
  if constexpr (MODE == VFML_COLORIZE_HSV) {
    f.x = hsv_clean(f.x);
    f.y = hsv_clean(f.y);
  }
  const float xx = f.x * f.x, yy = f.y * f.y;
  return root32(xx + yy);
}

// the maximum as an ordered u32: non-negative floats order like their bit patterns; any NaN becomes the canonical
// quiet NaN (above +inf), which is what numpy's / torch's max returns then
template <int MODE>
__global__ void colorize_max_kernel(const float2* __restrict__ flow, int64_t n, unsigned* __restrict__ cell) {
  unsigned m = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const float v = magnitude<MODE>(flow[p]);
    const unsigned b = v != v ? 0x7fc00000u : __float_as_uint(v);
    m = b > m ? b : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_down(m, off, 64);
    m = o > m ? o : m;
  }
  __shared__ unsigned wave_max[4];                         // one atomic per block, not per wavefront
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) m = wave_max[k] > m ? wave_max[k] : m;
    if (m != 0) atomicMax(cell, m);
  }
}

// OpenCV's sector table (HSV2RGB_native): b, g, r = tab[sector_data[sector][0..2]]
__constant__ unsigned char kSector[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};

// saturate_cast<uchar>(x * 255): round half to even, clamp to [0, 255]
__device__ __forceinline__ unsigned char sat_u8(float x) {
#pragma clang fp contract(off)
  const float r = rintf(x * 255.0f);
  return (unsigned char)(r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r));
}

// Middlebury colour wheel of torchvision.utils.flow_to_image: RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 (55 entries)
__device__ __forceinline__ void wheel_entry(int k, float (&c)[3]) {
  int r, g, b;
  if (k < 15) { r = 255; g = 255 * k / 15; b = 0; }
  else if (k < 21) { k -= 15; r = 255 - 255 * k / 6; g = 255; b = 0; }
  else if (k < 25) { k -= 21; r = 0; g = 255; b = 255 * k / 4; }
  else if (k < 36) { k -= 25; r = 0; g = 255 - 255 * k / 11; b = 255; }
  else if (k < 49) { k -= 36; r = 255 * k / 13; g = 0; b = 255; }
  else { k -= 49; r = 255; g = 0; b = 255 - 255 * k / 6; }
  c[0] = (float)r; c[1] = (float)g; c[2] = (float)b;
}

template <int MODE>
__global__ void colorize_kernel(const float2* __restrict__ flow, int64_t n, const unsigned* __restrict__ cell,
                                unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
  const float mx = __uint_as_float(*cell);
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    float2 f = flow[p];
    unsigned char rgb[3];
    if constexpr (MODE == VFML_COLORIZE_HSV) {
      f.x = hsv_clean(f.x);
      f.y = hsv_clean(f.y);
      const float mag = magnitude<VFML_COLORIZE_HSV>(f);
      float hue = div32(atan2_32(f.y, f.x) + kPi32, kTwoPi32) * 180.0f;
      hue = hue != hue ? hue : fminf(fmaxf(hue, 0.0f), 180.0f);
      const unsigned char H = u8_trunc(hue);
      const unsigned char S = mx > 0.0f ? u8_trunc(div32(mag, mx) * 255.0f) : (unsigned char)0;
      // HSV2RGB of the 8-bit triple (H, S, 255), DESIGN.md section 9
      const float s = div32((float)S, 255.0f), v = 1.0f;
      float h = (float)H * (6.0f / 180.0f);
      while (h >= 6.0f) h -= 6.0f;
      int sector = (int)floorf(h);
      h -= (float)sector;
      if ((unsigned)sector >= 6u) { sector = 0; h = 0.0f; }
      float tab[4];
      tab[0] = v;
      tab[1] = v * (1.0f - s);
      tab[2] = v * (1.0f - s * h);
      tab[3] = v * (1.0f - s * (1.0f - h));
      const float b = S == 0 ? v : tab[kSector[sector][0]];
      const float g = S == 0 ? v : tab[kSector[sector][1]];
      const float r = S == 0 ? v : tab[kSector[sector][2]];
      rgb[0] = sat_u8(r); rgb[1] = sat_u8(g); rgb[2] = sat_u8(b);
    } else {
      const float denom = mx + kFltEps;
      const float nu = div32(f.x, denom), nv = div32(f.y, denom);
      const float rad = magnitude<VFML_COLORIZE_WHEEL>(make_float2(nu, nv));
      const float a = div32(atan2_32(-nv, -nu), kPi32);
      const float fk = div32(a + 1.0f, 2.0f) * 54.0f;
      int k0 = fk == fk ? (int)floorf(fk) : 0;
      k0 = k0 < 0 ? 0 : (k0 > 54 ? 54 : k0);                 // fk is in [0, 54] for every finite input
      const int k1 = k0 + 1 == 55 ? 0 : k0 + 1;
      const float fr = fk - (float)k0;
      float c0[3], c1[3];
      wheel_entry(k0, c0);
      wheel_entry(k1, c1);
      for (int c = 0; c < 3; ++c) {
        const float col0 = div32(c0[c], 255.0f), col1 = div32(c1[c], 255.0f);
        float col = (1.0f - fr) * col0 + fr * col1;
        col = 1.0f - rad * (1.0f - col);
        // flow_to_image's floor(255 * col) as uint8, then the reference wrapper's uint8 `* 255` (wraps mod 256)
        const unsigned char x = u8_trunc(floorf(255.0f * col));
        rgb[c] = (unsigned char)(x * 255u);
      }
    }
    out[3 * p] = rgb[0];
    out[3 * p + 1] = rgb[1];
    out[3 * p + 2] = rgb[2];
  }
}

// ---- external flow (--flow-input): decode and difference overlay -------------------------------------------------------
// MotionVectorsRG8FlowEncoder.decode / MotionVectorsRGB8FlowEncoder.decode ('rgb+'), step by step in float32
template <int MODE>
__global__ void flow_decode_kernel(const unsigned char* __restrict__ enc, int64_t n, float clamp,
                                   float2* __restrict__ out) {
#pragma clang fp contract(off)
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const float nr = div32((float)enc[3 * p], 255.0f), ng = div32((float)enc[3 * p + 1], 255.0f);
    float2 f;
    if constexpr (MODE == VFML_ENCODE_RG8) {
      f.x = (nr * 2.0f) * clamp - clamp;
      f.y = (ng * 2.0f) * clamp - clamp;
    } else {
      const float nb = div32((float)enc[3 * p + 2], 255.0f);
      const float dx = nr * 2.0f - 1.0f, dy = ng * 2.0f - 1.0f;
      const float xx = dx * dx, yy = dy * dy, bb = nb * nb;
      const float mag = div32(1.0f, root32((xx + yy) + bb)) * clamp;
      f.x = dx * mag;
      f.y = dy * mag;
    }
    out[p] = f;
  }
}

// radar colours of the difference classes, R | G << 8 | B << 16: green, yellow, orange, red, magenta
__device__ __forceinline__ unsigned radar_colour(int k) {
  return k == 0 ? 0x00ff00u : k == 1 ? 0x00ffffu : k == 2 ? 0x00a5ffu : k == 3 ? 0x0000ffu : 0xff00ffu;
}

__global__ void diff_overlay_kernel(const float2* __restrict__ fa, const float2* __restrict__ fb, int h, int w,
                                    unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)h * w;
  const int y0 = h - 20;                                   // the legend's base line
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const float2 a = fa[p], b = fb[p];
    const float dx = a.x - b.x, dy = a.y - b.y;
    const float xx = dx * dx, yy = dy * dy;
    const float m = root32(xx + yy);
    unsigned rgb = 0;                                      // NaN matches no class: black
    if (m <= 0.1f) rgb = radar_colour(0);
    else if (m <= 0.5f) rgb = radar_colour(1);
    else if (m <= 1.0f) rgb = radar_colour(2);
    else if (m <= 2.0f) rgb = radar_colour(3);
    else if (m > 2.0f) rgb = radar_colour(4);
    // legend square i: white (x-1, y0-13)..(x+13, y0+1), colour (x, y0-12)..(x+12, y0), x = 10 + 45 i, corners inclusive
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const int lx = x - 9;
    if (lx >= 0 && y >= y0 - 13 && y <= y0 + 1) {
      const int i = lx / 45, r = lx - 45 * i;
      if (i < 5 && r <= 14) {
        rgb = 0xffffffu;
        if (r >= 1 && r <= 13 && y >= y0 - 12 && y <= y0) rgb = radar_colour(i);
      }
    }
    out[3 * p] = (unsigned char)rgb;
    out[3 * p + 1] = (unsigned char)(rgb >> 8);
    out[3 * p + 2] = (unsigned char)(rgb >> 16);
  }
}

// ---- frame composer ---------------------------------------------------------------------------------------------------
struct ComposeArgs {
  const void* tile[6];
  int type[6];
  int h, w;               // tile size
  int ow, oh;             // output frame in pixels
  int layout, bgr, bottom_up;
  int64_t stride;         // output row stride, bytes
  int words;              // dwords per output row, rounded up
  unsigned char* out;
};

__device__ __forceinline__ unsigned char tile_byte(const ComposeArgs& a, int t, int64_t idx) {
  const int ty = a.type[t];
  if (ty == VFML_PIX_U8) return ((const unsigned char*)a.tile[t])[idx];
  // np.clip(x, 0, 255).astype(np.uint8); NaN -> 0
  if (ty == VFML_PIX_F32) {
    const float v = ((const float*)a.tile[t])[idx];
    return v != v ? (unsigned char)0 : u8_trunc(fminf(fmaxf(v, 0.0f), 255.0f));
  }
  const double v = ((const double*)a.tile[t])[idx];
  return v != v ? (unsigned char)0 : u8_trunc64(fmin(fmax(v, 0.0), 255.0));
}

__device__ __forceinline__ unsigned char out_byte(const ComposeArgs& a, int y, int64_t col) {
  if (col >= 3 * (int64_t)a.ow) return 0;                  // DIB row padding
  const int x = (int)(col / 3), c = (int)(col - 3 * (int64_t)x);
  int t = 0, sy = y, sx = x;
  if (a.layout == VFML_COMPOSE_SIDE_BY_SIDE) {
    t = x >= a.w;
    sx = x - t * a.w;
  } else if (a.layout == VFML_COMPOSE_STACKED) {
    t = y >= a.h;
    sy = y - t * a.h;
  } else {                                                 // GRID_2X2 and GRID_2X3: two tiles per tile row
    const int tx = x >= a.w, tyy = (y >= a.h) + (y >= 2 * a.h);
    t = 2 * tyy + tx;
    sx = x - tx * a.w;
    sy = y - tyy * a.h;
  }
  const int sc = a.bgr ? 2 - c : c;
  return tile_byte(a, t, ((int64_t)sy * a.w + sx) * 3 + sc);
}

__global__ void compose_kernel(const ComposeArgs a) {
  const int row = blockIdx.y;
  const int y = a.bottom_up ? a.oh - 1 - row : row;
  unsigned char* dst = a.out + (int64_t)row * a.stride;
  for (int wd = blockIdx.x * blockDim.x + threadIdx.x; wd < a.words; wd += gridDim.x * blockDim.x) {
    const int64_t b0 = 4 * (int64_t)wd;
    if (b0 + 4 <= a.stride && (((uintptr_t)(dst + b0)) & 3u) == 0) {
      unsigned v = 0;
      for (int k = 0; k < 4; ++k) v |= (unsigned)out_byte(a, y, b0 + k) << (8 * k);
      *(unsigned*)(dst + b0) = v;
    } else {
      for (int k = 0; k < 4 && b0 + k < a.stride; ++k) dst[b0 + k] = out_byte(a, y, b0 + k);
    }
  }
}

}  // namespace

extern "C" int vfml_flow_colorize(const float* flow, int h, int w, int mode, void* workspace, unsigned char* out,
                                  void* stream) {
  VFML_REQUIRE(flow && workspace && out && h > 0 && w > 0, "vfml_flow_colorize: bad argument");
  VFML_REQUIRE(mode == VFML_COLORIZE_HSV || mode == VFML_COLORIZE_WHEEL, "vfml_flow_colorize: unknown mode %d", mode);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(flow) & 7u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0,
               "vfml_flow_colorize: flow must be 8-byte and workspace 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned* cell = reinterpret_cast<unsigned*>(workspace);
  if (hipMemsetAsync(cell, 0, sizeof(unsigned), s) != hipSuccess) return vfml_check_launch("vfml_flow_colorize");
  const int64_t n = (int64_t)h * w;
  const float2* f2 = reinterpret_cast<const float2*>(flow);
  const dim3 block(256);
  const dim3 rgrid(blocks_for(n, 4 * 256));                // 4 pixels per thread, 256 threads (4 wavefronts)
  const dim3 grid(blocks_for(n, 256));
  if (mode == VFML_COLORIZE_HSV) {
    hipLaunchKernelGGL(colorize_max_kernel<VFML_COLORIZE_HSV>, rgrid, block, 0, s, f2, n, cell);
    hipLaunchKernelGGL(colorize_kernel<VFML_COLORIZE_HSV>, grid, block, 0, s, f2, n, cell, out);
  } else {
    hipLaunchKernelGGL(colorize_max_kernel<VFML_COLORIZE_WHEEL>, rgrid, block, 0, s, f2, n, cell);
    hipLaunchKernelGGL(colorize_kernel<VFML_COLORIZE_WHEEL>, grid, block, 0, s, f2, n, cell, out);
  }
  return vfml_check_launch("vfml_flow_colorize");
}

extern "C" int vfml_flow_decode(const unsigned char* encoded, int h, int w, int mode, float clamp, float* flow,
                                void* stream) {
  VFML_REQUIRE(encoded && flow && h > 0 && w > 0, "vfml_flow_decode: bad argument");
  VFML_REQUIRE(mode == VFML_ENCODE_RG8 || mode == VFML_ENCODE_RGB8, "vfml_flow_decode: unknown mode %d", mode);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(flow) & 7u) == 0, "vfml_flow_decode: flow must be 8-byte aligned");
  const int64_t n = (int64_t)h * w;
  float2* f2 = reinterpret_cast<float2*>(flow);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 block(256), grid(blocks_for(n, 256));
  if (mode == VFML_ENCODE_RG8)
    hipLaunchKernelGGL(flow_decode_kernel<VFML_ENCODE_RG8>, grid, block, 0, s, encoded, n, clamp, f2);
  else
    hipLaunchKernelGGL(flow_decode_kernel<VFML_ENCODE_RGB8>, grid, block, 0, s, encoded, n, clamp, f2);
  return vfml_check_launch("vfml_flow_decode");
}

extern "C" int vfml_flow_diff_overlay(const float* flow_a, const float* flow_b, int h, int w, unsigned char* out,
                                      void* stream) {
  VFML_REQUIRE(flow_a && flow_b && out && h > 0 && w > 0, "vfml_flow_diff_overlay: bad argument");
  VFML_REQUIRE(((reinterpret_cast<uintptr_t>(flow_a) | reinterpret_cast<uintptr_t>(flow_b)) & 7u) == 0,
               "vfml_flow_diff_overlay: flows must be 8-byte aligned");
  hipLaunchKernelGGL(diff_overlay_kernel, dim3(blocks_for((int64_t)h * w, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float2*>(flow_a),
                     reinterpret_cast<const float2*>(flow_b), h, w, out);
  return vfml_check_launch("vfml_flow_diff_overlay");
}

extern "C" int vfml_compose_frame(const void* const* tiles, const int* tile_types, int h, int w, int layout, int flags,
                                  int64_t row_stride, unsigned char* out, void* stream) {
  VFML_REQUIRE(tiles && tile_types && out && h > 0 && w > 0, "vfml_compose_frame: bad argument");
  VFML_REQUIRE(layout == VFML_COMPOSE_SIDE_BY_SIDE || layout == VFML_COMPOSE_STACKED ||
                   layout == VFML_COMPOSE_GRID_2X2 || layout == VFML_COMPOSE_GRID_2X3,
               "vfml_compose_frame: unknown layout %d", layout);
  VFML_REQUIRE((flags & ~(VFML_COMPOSE_BGR | VFML_COMPOSE_BOTTOM_UP)) == 0, "vfml_compose_frame: unknown flags 0x%x",
               flags);
  ComposeArgs a;
  const int nt = layout == VFML_COMPOSE_GRID_2X3 ? 6 : (layout == VFML_COMPOSE_GRID_2X2 ? 4 : 2);
  for (int t = 0; t < 6; ++t) {
    a.tile[t] = t < nt ? tiles[t] : nullptr;
    a.type[t] = t < nt ? tile_types[t] : VFML_PIX_U8;
    if (t < nt) {
      VFML_REQUIRE(a.tile[t], "vfml_compose_frame: tile %d missing", t);
      VFML_REQUIRE(a.type[t] == VFML_PIX_U8 || a.type[t] == VFML_PIX_F32 || a.type[t] == VFML_PIX_F64,
                   "vfml_compose_frame: tile %d has unknown type %d", t, a.type[t]);
    }
  }
  a.h = h; a.w = w;
  a.ow = layout == VFML_COMPOSE_STACKED ? w : 2 * w;
  a.oh = layout == VFML_COMPOSE_SIDE_BY_SIDE ? h : (layout == VFML_COMPOSE_GRID_2X3 ? 3 * h : 2 * h);
  VFML_REQUIRE(row_stride >= 3 * (int64_t)a.ow && row_stride < ((int64_t)1 << 31),
               "vfml_compose_frame: row stride %lld below 3 * %d", (long long)row_stride, a.ow);
  VFML_REQUIRE(a.oh <= 65535, "vfml_compose_frame: output height %d above the grid's y limit", a.oh);
  a.layout = layout;
  a.bgr = (flags & VFML_COMPOSE_BGR) != 0;
  a.bottom_up = (flags & VFML_COMPOSE_BOTTOM_UP) != 0;
  a.stride = row_stride;
  a.words = (int)((row_stride + 3) / 4);
  a.out = out;
  const int bx = (a.words + 255) / 256;
  hipLaunchKernelGGL(compose_kernel, dim3(bx, a.oh), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return vfml_check_launch("vfml_compose_frame");
}
