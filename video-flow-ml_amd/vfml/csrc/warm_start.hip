// forward_interpolate: a 1/8-resolution flow projected forward along itself, the warm start of the next field of a MemFlow
// stream (include/vfml.h vfml_flow_forward_interpolate).  Upstream does this on the host with a k-d tree
// (scipy griddata, method 'nearest'); here it is a brute-force nearest-neighbour search, exact by construction:
//   pass 1  a workgroup owns FI_TARGETS target cells, one per lane, and one chunk of FI_CHUNK source cells, whose landing
//           points it streams through LDS in tiles of FI_TILE; a source that lands outside the frame is staged as a point at
//           infinity.  A lane keeps the least squared distance and its source in registers; sources come in rising index
//           order and only a strictly smaller distance replaces the held one, so a tie stays with the lowest index.  The
//           lane's partial minimum goes to a [chunks][P] slab as the 64-bit key (bits of d2, index).
//   pass 2  per target cell the least key over the chunks (an integer minimum: no order of summation, the same bits every
//           run), then the gather of that source's flow.
// Every float operation is a single rounded one, as the numpy oracle does it: no contraction to a fused multiply-add.
#include "vfml_common.h"

namespace {
#pragma clang fp contract(off)

constexpr int FI_TARGETS = 256;    // target cells per workgroup = its threads
constexpr int FI_TILE = 256;       // source cells staged in LDS at a time (one per thread)
constexpr int FI_CHUNK = 2048;     // source cells per workgroup (grid.y walks the chunks)
static_assert(FI_TILE == FI_TARGETS && FI_CHUNK % FI_TILE == 0, "a thread stages one source per tile; whole tiles per chunk");
constexpr unsigned long long FI_NONE = ~0ull;      // no valid source (above every key of a finite distance)

__global__ __launch_bounds__(FI_TARGETS) void forward_interpolate_search_kernel(const float* __restrict__ flow, int ld_in, int h,
                                                                              int w, int P, int chunks,
                                                                              unsigned long long* __restrict__ slab) {
#pragma clang fp contract(off)
  __shared__ float2 land[FI_TILE];
  const int map = blockIdx.z, chunk = blockIdx.y;
  const int t = blockIdx.x * FI_TARGETS + threadIdx.x;          // the lane's target cell (past P: computed, not stored)
  const float tx = (float)(t % w), ty = (float)(t / w);
  const float fw = (float)w, fh = (float)h;
  const float* f = flow + (int64_t)map * P * ld_in;
  const int s_end = min(P, (chunk + 1) * FI_CHUNK);
  float best = INFINITY;
  int best_at = -1;
  for (int s0 = chunk * FI_CHUNK; s0 < s_end; s0 += FI_TILE) {
    const int s = s0 + threadIdx.x;
    float2 p = make_float2(INFINITY, 0.f);                      // an invalid source: at infinite distance from every cell
    if (s < s_end) {
      const float x1 = (float)(s % w) + f[(int64_t)s * ld_in];
      const float y1 = (float)(s / w) + f[(int64_t)s * ld_in + 1];
      if (x1 > 0.f && x1 < fw && y1 > 0.f && y1 < fh) p = make_float2(x1, y1);      // (NaN and infinities fail these)
    }
    __syncthreads();                                            // the previous tile has been read
    land[threadIdx.x] = p;
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < FI_TILE; ++j) {                         // (tile entries past s_end are points at infinity)
      const float2 q = land[j];
      const float dx = q.x - tx, dy = q.y - ty;
      const float d2 = dx * dx + dy * dy;
      if (d2 < best) {
        best = d2;
        best_at = s0 + j;
      }
    }
  }
  if (t < P) {
    // distances of valid sources are finite and non-negative: their bits order as the numbers do
    const unsigned long long key = best_at < 0 ? FI_NONE
                                               : ((unsigned long long)__builtin_bit_cast(unsigned, best) << 32) | (unsigned)best_at;
    slab[((int64_t)map * chunks + chunk) * P + t] = key;
  }
}

__global__ void forward_interpolate_gather_kernel(const float* __restrict__ flow, int ld_in, int P, int chunks, int64_t total,
                                                  const unsigned long long* __restrict__ slab, float* __restrict__ out, int ld_out,
                                                  int32_t* __restrict__ index) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t map = i / P;
    const int t = (int)(i - map * P);
    const unsigned long long* k = slab + map * chunks * P + t;
    unsigned long long key = FI_NONE;
    for (int c = 0; c < chunks; ++c) {
      const unsigned long long v = k[(int64_t)c * P];
      key = v < key ? v : key;
    }
    const int at = key == FI_NONE ? -1 : (int)(unsigned)key;
    float fx = 0.f, fy = 0.f;
    if (at >= 0) {
      const float* f = flow + (map * P + at) * ld_in;
      fx = f[0];
      fy = f[1];
    }
    float* o = out + i * ld_out;
    o[0] = fx;
    o[1] = fy;
    if (ld_out >= 4) o[2] = o[3] = 0.f;
    if (index) index[i] = at;
  }
}

inline int fi_chunks(int64_t P) { return (int)((P + FI_CHUNK - 1) / FI_CHUNK); }
constexpr int64_t FI_MAX_CELLS = 1 << 24;      // cell coordinates are exact in f32; 65535 * FI_CHUNK chunks would allow more

}  // namespace

extern "C" int64_t vfml_flow_forward_interpolate_workspace_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1 || (int64_t)h * w > FI_MAX_CELLS) return 0;
  const int64_t P = (int64_t)h * w;
  return (int64_t)n * fi_chunks(P) * P * 8;
}

extern "C" int vfml_flow_forward_interpolate(const float* flow, int ld_in, int n, int h, int w, float* out, int ld_out,
                                             int32_t* index, void* workspace, int64_t workspace_bytes, void* stream) {
  VFML_REQUIRE(flow && out && workspace, "vfml_flow_forward_interpolate: null pointer");
  VFML_REQUIRE(n >= 1 && n <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= FI_MAX_CELLS,
               "vfml_flow_forward_interpolate: n = %d maps (1..65535) of h = %d, w = %d (at least 1, at most 2^24 cells)", n, h, w);
  VFML_REQUIRE(ld_in >= 2 && ld_out >= 2, "vfml_flow_forward_interpolate: ld_in = %d, ld_out = %d (at least 2 floats per cell)",
               ld_in, ld_out);
  const int P = h * w;
  const int chunks = fi_chunks(P);
  const int64_t total = (int64_t)n * P;
  const int64_t need = total * chunks * 8;
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= need,
               "vfml_flow_forward_interpolate: workspace of %lld bytes, 8-byte aligned (got %lld)", (long long)need,
               (long long)workspace_bytes);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(flow) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 &&
               (reinterpret_cast<uintptr_t>(index) & 3u) == 0, "vfml_flow_forward_interpolate: 4-byte alignment");
  const char* a0 = reinterpret_cast<const char*>(flow);
  const char* b0 = reinterpret_cast<const char*>(out);
  VFML_REQUIRE(a0 + total * ld_in * 4 <= b0 || b0 + total * ld_out * 4 <= a0,
               "vfml_flow_forward_interpolate: out overlaps flow (the gather reads flow while out is written)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* slab = reinterpret_cast<unsigned long long*>(workspace);
  hipLaunchKernelGGL(forward_interpolate_search_kernel, dim3((P + FI_TARGETS - 1) / FI_TARGETS, chunks, n), dim3(FI_TARGETS), 0, st,
                     flow, ld_in, h, w, P, chunks, slab);
  int rc = vfml_check_launch("vfml_flow_forward_interpolate");
  if (rc) return rc;
  const int64_t g = (total + 255) / 256;
  hipLaunchKernelGGL(forward_interpolate_gather_kernel, dim3((int)(g > 8192 ? 8192 : g)), dim3(256), 0, st, flow, ld_in, P, chunks,
                     total, slab, out, ld_out, index);
  return vfml_check_launch("vfml_flow_forward_interpolate");
}
