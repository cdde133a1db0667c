// Scene-cut statistic of uint8 RGB frames (tests/scene_cut_oracle.py is the definition): per frame a
// signature S[16][64] - the count of pixels per cell of a 4x4 grid and per bin Y >> 2 of the integer luma
// Y = (77 R + 150 G + 29 B + 128) >> 8 - and the distance d[t] = sum |S_t - S_{t-1}| of consecutive signatures.
// Launches, all on the caller's stream:
//   1. hipMemsetAsync        the n signatures
//   2. scene_signature       a workgroup takes a few rows of ONE cell of one frame: 64 bins x 32 copies in LDS (a thread
//                            adds to copy tid & 31, so a frame of one colour spreads over 32 addresses instead of one), the
//                            packed RGB rows read as whole dwords - three dwords are four pixels - where the address allows
//                            and byte by byte at the row ends; its non-zero bins go to the frame's signature with one
//                            integer atomic each (the pattern of turbulence.hip's histogram)
//   3. scene_distance        a workgroup per frame: 1024 absolute differences, summed
// All sums are integer: the result does not depend on the order of arrival, and is the same bytes on every run.
#include "vfml_common.h"

namespace {

constexpr int NT = 256, BINS = 64, CELLS = 16, COPIES = 32, SIG = CELLS * BINS;
constexpr int BLOCK_PIXELS = 8192;       // pixels a signature workgroup aims at

struct SigArgs {
  const unsigned char* frames;   // [n][H][W][3]
  unsigned* sig;                 // [n][SIG]
  int H, W;
  int rows_per_block;            // rows of a cell one workgroup takes
  int stride;                    // work items per row: the row's dword groups, then its head and tail pixels
  int shift;                     // pixels by which a group of four is moved so that its first byte is dword aligned
};

__device__ __forceinline__ unsigned luma_bin(unsigned r, unsigned g, unsigned b) {
  return ((77u * r + 150u * g + 29u * b + 128u) >> 8) >> 2;
}

// first row / column of cell c along an axis of n pixels: the smallest p with p * 4 / n == c
__device__ __forceinline__ int cell_begin(int c, int n) { return (int)(((int64_t)c * n + 3) >> 2); }

__global__ void __launch_bounds__(NT) scene_signature_kernel(const SigArgs a) {
  __shared__ unsigned hist[BINS * COPIES];
  const int tid = threadIdx.x;
  const int cell = blockIdx.y, cy = cell >> 2, cx = cell & 3;
  const int y_lo = cell_begin(cy, a.H) + (int)blockIdx.x * a.rows_per_block;
  const int y_hi = min(cell_begin(cy + 1, a.H), y_lo + a.rows_per_block);
  const int x0 = cell_begin(cx, a.W), x1 = cell_begin(cx + 1, a.W);
  if (y_lo >= y_hi || x0 >= x1) return;                 // uniform: nothing of this cell here (or an empty cell)
  for (int i = tid; i < BINS * COPIES; i += NT) hist[i] = 0;
  __syncthreads();

  const int64_t frame_px = (int64_t)blockIdx.z * a.H * a.W;
  // pixel v of the shifted numbering starts at byte 3 * (v - shift) of `frames`; v % 4 == 0 is a dword-aligned address
  const unsigned* words = reinterpret_cast<const unsigned*>(a.frames - 3 * a.shift);
  unsigned* mine = hist + (tid & (COPIES - 1));
  const int items = (y_hi - y_lo) * a.stride;
  for (int i = tid; i < items; i += NT) {
    const int row = i / a.stride, it = i - row * a.stride;
    const int64_t v0 = frame_px + (int64_t)(y_lo + row) * a.W + x0 + a.shift, v1 = v0 + (x1 - x0);
    int64_t gb = (v0 + 3) >> 2, ge = v1 >> 2;           // whole groups [gb, ge)
    int64_t head_end = gb << 2, tail_begin = ge << 2;
    if (ge <= gb) { ge = gb; head_end = v1; tail_begin = v1; }     // the row lies inside one or two partial groups
    const int groups = (int)(ge - gb), head = (int)(head_end - v0), tail = (int)(v1 - tail_begin);
    if (it < groups) {
      const unsigned* p = words + 3 * (gb + it);
      const unsigned d0 = p[0], d1 = p[1], d2 = p[2];
      const unsigned b0 = luma_bin(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u);
      const unsigned b1 = luma_bin(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u);
      const unsigned b2 = luma_bin((d1 >> 16) & 255u, d1 >> 24, d2 & 255u);
      const unsigned b3 = luma_bin((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24);
      if (b0 == b1 && b1 == b2 && b2 == b3) {           // (the common case in a smooth picture: one LDS atomic, not four)
        atomicAdd(mine + b0 * COPIES, 4u);
      } else {
        atomicAdd(mine + b0 * COPIES, 1u);
        atomicAdd(mine + b1 * COPIES, 1u);
        atomicAdd(mine + b2 * COPIES, 1u);
        atomicAdd(mine + b3 * COPIES, 1u);
      }
    } else if (it - groups < head + tail) {
      const int j = it - groups;
      const int64_t v = j < head ? v0 + j : tail_begin + (j - head);
      const unsigned char* p = a.frames + 3 * (v - a.shift);
      atomicAdd(mine + luma_bin(p[0], p[1], p[2]) * COPIES, 1u);
    }
  }
  __syncthreads();
  if (tid < BINS) {
    unsigned c = 0;
    for (int j = 0; j < COPIES; ++j) c += hist[tid * COPIES + ((j + tid) & (COPIES - 1))];
    if (c) atomicAdd(a.sig + (int64_t)blockIdx.z * SIG + cell * BINS + tid, c);
  }
}

// d[t] = sum over the 1024 counts of |S_t - S_{t-1}|; frame 0 against prev_sig, or 0 without one.  At most 2 H W < 2^32.
__global__ void __launch_bounds__(NT) scene_distance_kernel(const unsigned* sig, const unsigned* prev_sig, unsigned* dist) {
  __shared__ unsigned part[NT / 64];
  const int t = blockIdx.x, tid = threadIdx.x;
  const unsigned* cur = sig + (int64_t)t * SIG;
  const unsigned* prev = t > 0 ? cur - SIG : prev_sig;
  unsigned s = 0;
  if (prev) {
    for (int i = tid; i < SIG; i += NT) {
      const unsigned x = cur[i], y = prev[i];
      s += x > y ? x - y : y - x;
    }
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    unsigned total = 0;
    for (int w = 0; w < NT / 64; ++w) total += part[w];
    dist[t] = total;
  }
}

}  // namespace

extern "C" int vfml_scene_distances(const unsigned char* frames, int n, int H, int W, const uint32_t* prev_sig,
                                    uint32_t* sig_out, uint32_t* dist_out, void* stream) {
  VFML_REQUIRE(frames && sig_out && dist_out, "vfml_scene_distances: null frames / sig_out / dist_out");
  VFML_REQUIRE(n >= 1 && n <= 65535, "vfml_scene_distances: %d frames (1..65535 per call)", n);
  VFML_REQUIRE(H >= 1 && W >= 1, "vfml_scene_distances: empty frame %dx%d", W, H);
  VFML_REQUIRE((int64_t)H * W < (1ll << 31), "vfml_scene_distances: frame %dx%d has 2^31 pixels or more", W, H);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(sig_out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(dist_out) & 3u) == 0 &&
               (reinterpret_cast<uintptr_t>(prev_sig) & 3u) == 0,
               "vfml_scene_distances: prev_sig / sig_out / dist_out must be 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);

  SigArgs a;
  a.frames = frames; a.sig = sig_out; a.H = H; a.W = W;
  const int cell_w = (W + 3) / 4, cell_h = (H + 3) / 4;            // the largest cell
  a.rows_per_block = (BLOCK_PIXELS + cell_w - 1) / cell_w;
  if (a.rows_per_block > cell_h) a.rows_per_block = cell_h;
  a.stride = cell_w / 4 + 8;               // at most cell_w / 4 groups, and at most 6 head and tail pixels
  // frames + 3 k is dword aligned for k = 3 (frames mod 4) mod 4: the group of pixels -k .. 3 - k starts there
  a.shift = (int)((3u * (reinterpret_cast<uintptr_t>(frames) & 3u)) & 3u);
  const int chunks = (cell_h + a.rows_per_block - 1) / a.rows_per_block;
  VFML_REQUIRE(chunks <= 65535, "vfml_scene_distances: frame %dx%d needs %d row blocks per cell", W, H, chunks);

  const hipError_t e = hipMemsetAsync(sig_out, 0, sizeof(uint32_t) * SIG * (size_t)n, s);
  if (e != hipSuccess) {
    vfml_set_error("vfml_scene_distances: hipMemsetAsync: %s", hipGetErrorString(e));
    return 2;
  }
  hipLaunchKernelGGL(scene_signature_kernel, dim3((unsigned)chunks, CELLS, (unsigned)n), dim3(NT), 0, s, a);
  hipLaunchKernelGGL(scene_distance_kernel, dim3((unsigned)n), dim3(NT), 0, s, (const unsigned*)sig_out,
                     (const unsigned*)prev_sig, (unsigned*)dist_out);
  return vfml_check_launch("vfml_scene_distances");
}
