// vfml_resize_u8: the uint8 picture resize behind --fast: OpenCV's 8-bit
// INTER_LINEAR scheme as this project defines it - a 2x2 mean when both sides halve exactly, else a separable two-tap
// filter in 11-bit fixed point.  Integer arithmetic only: the float work (tap positions, weights) is done once on the
// host into two tables of (s, s1, a0, a1) rows that the CPU path and this kernel both read, so the two cannot round
// differently.
//
// One thread owns four neighbouring output pixels of one row = 12 bytes, stored as three dwords where the run is whole
// and 4-byte aligned and byte by byte elsewhere (row tails, rows of an odd width).  A block works on one output row: the
// row's y taps are block-uniform, a thread's four x-table rows are four 16-byte loads ahead of the pixel loop, and the
// pixel loop itself touches source bytes only.  The kernel is latency- and bandwidth-bound (at most four source pixels
// per output pixel); taps are clamped to the picture on the device, so whatever a table holds no access leaves it.
#include "vfml_common.h"

namespace {

constexpr int kRun = 4;                   // output pixels per thread

struct ResizeArgs {
  const unsigned char* src;
  unsigned char* dst;
  int n, H, W, h, w;
  int64_t sstride, dstride;               // bytes between frames
  const int4* xtab;
  const int4* ytab;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// 12 bytes -> the thread's run of a row: whole dwords where the row allows
__device__ __forceinline__ void store_run(unsigned char* p, const unsigned (&b)[3 * kRun], int npx) {
  if (npx == kRun && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
    unsigned* q = reinterpret_cast<unsigned*>(p);
#pragma unroll
    for (int d = 0; d < 3; ++d) q[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 3 * kRun; ++k)
      if (k < 3 * npx) p[k] = (unsigned char)b[k];
  }
}

template <bool AREA>
__global__ void resize_u8_kernel(const ResizeArgs a) {
  const int x0 = kRun * (blockIdx.x * blockDim.x + threadIdx.x);
  if (x0 >= a.w) return;
  const int npx = a.w - x0 < kRun ? a.w - x0 : kRun;
  const int y = blockIdx.y;
  unsigned b[3 * kRun];
  if constexpr (AREA) {
    for (int f = blockIdx.z; f < a.n; f += gridDim.z) {
      const unsigned char* r0 = a.src + f * a.sstride + (int64_t)(2 * y) * (3 * a.W) + 6 * x0;
      const unsigned char* r1 = r0 + 3 * a.W;
      unsigned t0[6 * kRun], t1[6 * kRun];
      if (npx == kRun && ((reinterpret_cast<uintptr_t>(r0) | reinterpret_cast<uintptr_t>(r1)) & 3u) == 0) {
#pragma unroll
        for (int d = 0; d < 6; ++d) {
          const unsigned u0 = reinterpret_cast<const unsigned*>(r0)[d], u1 = reinterpret_cast<const unsigned*>(r1)[d];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            t0[4 * d + k] = (u0 >> (8 * k)) & 255u;
            t1[4 * d + k] = (u1 >> (8 * k)) & 255u;
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < 6 * kRun; ++k) {
          const bool in = k < 6 * npx;
          t0[k] = in ? r0[k] : 0u;
          t1[k] = in ? r1[k] : 0u;
        }
      }
#pragma unroll
      for (int p = 0; p < kRun; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          b[3 * p + c] = (t0[6 * p + c] + t0[6 * p + 3 + c] + t1[6 * p + c] + t1[6 * p + 3 + c] + 2u) >> 2;
      store_run(a.dst + f * a.dstride + ((int64_t)y * a.w + x0) * 3, b, npx);
    }
  } else {
    const int4 ty = a.ytab[y];
    const int y0 = clampi(ty.x, a.H - 1), y1 = clampi(ty.y, a.H - 1), b0 = ty.z, b1 = ty.w;
    int xs[kRun], xs1[kRun], a0[kRun], a1[kRun];
#pragma unroll
    for (int p = 0; p < kRun; ++p) {
      const int4 tx = a.xtab[p < npx ? x0 + p : x0];
      xs[p] = 3 * clampi(tx.x, a.W - 1);
      xs1[p] = 3 * clampi(tx.y, a.W - 1);
      a0[p] = tx.z;
      a1[p] = tx.w;
    }
    for (int f = blockIdx.z; f < a.n; f += gridDim.z) {
      const unsigned char* r0 = a.src + f * a.sstride + (int64_t)y0 * (3 * a.W);
      const unsigned char* r1 = a.src + f * a.sstride + (int64_t)y1 * (3 * a.W);
#pragma unroll
      for (int p = 0; p < kRun; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int u0 = r0[xs[p] + c] * a0[p] + r0[xs1[p] + c] * a1[p];
          const int u1 = r1[xs[p] + c] * a0[p] + r1[xs1[p] + c] * a1[p];
          const int v = (((b0 * (u0 >> 4)) >> 16) + ((b1 * (u1 >> 4)) >> 16) + 2) >> 2;
          b[3 * p + c] = (unsigned)v & 255u;
        }
      store_run(a.dst + f * a.dstride + ((int64_t)y * a.w + x0) * 3, b, npx);
    }
  }
}

}  // namespace

extern "C" int vfml_resize_u8(const unsigned char* src, int n, int H, int W, int64_t src_frame_stride, unsigned char* dst,
                              int h, int w, int64_t dst_frame_stride, const int32_t* xtab, const int32_t* ytab,
                              void* stream) {
  VFML_REQUIRE(src && dst, "vfml_resize_u8: null picture");
  VFML_REQUIRE(n > 0 && H > 0 && W > 0 && h > 0 && w > 0, "vfml_resize_u8: bad size (n %d, %dx%d -> %dx%d)", n, W, H, w, h);
  VFML_REQUIRE(H <= 32768 && W <= 32768 && h <= 32768 && w <= 32768, "vfml_resize_u8: picture too large (side above 32768)");
  VFML_REQUIRE(src_frame_stride >= (int64_t)3 * H * W && dst_frame_stride >= (int64_t)3 * h * w,
               "vfml_resize_u8: frame stride below the frame's bytes");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (h == H && w == W) {                 // the picture unchanged
    const hipError_t e = hipMemcpy2DAsync(dst, (size_t)dst_frame_stride, src, (size_t)src_frame_stride, (size_t)3 * H * W,
                                          (size_t)n, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) {
      vfml_set_error("vfml_resize_u8: hipMemcpy2DAsync: %s", hipGetErrorString(e));
      return 2;
    }
    return 0;
  }
  const bool area = H == 2 * h && W == 2 * w;
  VFML_REQUIRE(area || (xtab && ytab), "vfml_resize_u8: null tap table (only the exact 2x2 case runs without)");
  VFML_REQUIRE(area || (vfml_aligned16(xtab) && vfml_aligned16(ytab)), "vfml_resize_u8: tap tables must be 16-byte aligned");
  ResizeArgs a;
  a.src = src, a.dst = dst, a.n = n, a.H = H, a.W = W, a.h = h, a.w = w;
  a.sstride = src_frame_stride, a.dstride = dst_frame_stride;
  a.xtab = reinterpret_cast<const int4*>(xtab), a.ytab = reinterpret_cast<const int4*>(ytab);
  const int runs = (w + kRun - 1) / kRun;
  const int block = runs <= 64 ? 64 : (runs <= 128 ? 128 : 256);
  const dim3 grid((runs + block - 1) / block, h, n < 1024 ? n : 1024);
  if (area)
    hipLaunchKernelGGL(resize_u8_kernel<true>, grid, dim3(block), 0, s, a);
  else
    hipLaunchKernelGGL(resize_u8_kernel<false>, grid, dim3(block), 0, s, a);
  return vfml_check_launch("vfml_resize_u8");
}
