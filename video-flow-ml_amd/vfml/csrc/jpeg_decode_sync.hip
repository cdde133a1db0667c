// vfml_jpeg_decode_rgb_sync, vfml_jpeg_decode_rgb_sync_sampled (the sampling as an argument): the
// JPEG decoder of jpeg_decode.hip with an entropy stage that does not need restart markers - the self-synchronising parallel Huffman decode: the scan is cut into subsequences
// of S raw bytes, one lane each, whatever the file's restart interval.  Same contract, same picture, same status bits as
// vfml_jpeg_decode_rgb; tests/jpeg_selfsync_oracle.py is the definition, jpeg_sync_steps.h the per-subsequence code
// (shared with tools/jpeg_sync_host.cpp, which runs it on the CPU under sanitizers).
//
// Eight launches and one memset on one stream, whatever the content, no synchronisation:
//   count, place   the marker kernels of jpeg_decode.hip: marker offsets by rank, count and sequence into the status cell
//   group          256 subsequences per workgroup.  speculate: every lane decodes its subsequence from block 0 / DC at
//                  its first bit; synchronise: a lane whose left neighbour's exit state is not the state it decoded from
//                  decodes again, until a round changes nothing (an LDS flag between barriers; at most 256 rounds)
//   chain          one workgroup walks the groups in order: the first subsequence of a group is decoded again from the
//                  last exit state of the group in front when that differs, the change is run through the group as above
//                  (rounds <= 256), and a segmented scan of the completed blocks gives every subsequence its first
//                  block (restarted behind a marker).  Groups: ceil(subsequences / 256), a count
//   memset         the coefficients
//   write          every lane decodes once more from its true entry state: non-zero AC coefficients to their natural
//                  place, the DC difference to place 0; the true chain's errors into the status cell
//   dc             a workgroup per interval: inclusive sums of the DC differences per component, low 16 bits kept
//                  (a template on the blocks per MCU: its sums index registers)
//   transform, colour   the picture kernels of jpeg_decode.hip, on the window's MCU rows
// The result is the fixed point of "entry state = the left neighbour's exit state", unique by induction from the known
// states (the scan's first bit, the byte behind a marker): exact whether or not speculation ever agrees; when it does
// not, the rounds of `group` are wasted and `chain` decodes one subsequence per round - the serial decoder's pace.
// LDS: the tables (3672 bytes: a first-level table on 8 bits per Huffman table, then limit / offset) plus the exchange
// arrays of a workgroup of 256 - 4704 bytes in group, 8800 in chain, 3672 in write: eight workgroups a CU by waves, not
// by LDS.  Per-lane table reads conflict on banks as the data has it; a lane's bytes come from its own cache lines (S is
// 1-8 lines).
#include "jpeg_decode_common.h"
#include "jpeg_sync_steps.h"

using namespace vfml_jpeg;
namespace js = vfml_jsync;

namespace {

#include "jpeg_tables.inc"

constexpr int kGroup = 256;               // subsequences per workgroup: the unit of the first synchronisation level

struct SyncArgs {
  DecArgs d;
  js::Rec* rec;                           // [subsequences]
  int* blk0;                              // [subsequences] first block of each
  long long nsub;
  int groups;
  int S;
};

__device__ __forceinline__ js::Ctx make_ctx(const SyncArgs& a) {
  js::Ctx c;
  c.scan = a.d.scan, c.n = a.d.n, c.mpos = a.d.mpos, c.nmark = (uint32_t)(a.d.nint - 1);
  c.ri = a.d.ri, c.nmcu = a.d.rows * a.d.cols, c.S = a.S, c.nb = a.d.nb, c.ny = a.d.ny;
  return c;
}

// One round of synchronisation in a workgroup: -> true when some lane decoded again.  Three barriers.
__device__ __forceinline__ bool sync_round(const js::Ctx& c, const js::Tabs& tabs, long long i, bool valid, uint32_t* exits,
                                           int* changed, js::Rec& r, bool& dirty) {
  const int tid = threadIdx.x;
  exits[tid] = r.exit;
  if (tid == 0) *changed = 0;
  __syncthreads();
  if (valid && tid > 0 && exits[tid - 1] != r.entry) {
    r.entry = exits[tid - 1];
    const js::Out o = js::decode_sub<false>(c, tabs, i, r.entry, 0, nullptr);
    r.exit = o.exit, r.nblk = o.nblk, r.mark = o.mark;
    dirty = true;
    *changed = 1;
  }
  __syncthreads();
  const bool any = *changed != 0;
  __syncthreads();
  return any;
}

__global__ __launch_bounds__(kGroup) void jpeg_sync_group_kernel(const SyncArgs a) {
  __shared__ js::Tabs tabs;
  __shared__ uint32_t exits[kGroup];
  __shared__ int changed;
  if ((*a.d.status & (kErrCount | kErrSequence)) != 0) return;       // set by `place` alone: the same for every lane
  js::tabs_fill(tabs, a.d.tables, kJpegZigzag, threadIdx.x, kGroup);
  __syncthreads();
  const js::Ctx c = make_ctx(a);
  const long long i = (long long)blockIdx.x * kGroup + threadIdx.x;
  const bool valid = i < a.nsub;
  js::Rec r = {0u, 0u, 0u, -1};
  if (valid) {
    const js::Out o = js::decode_sub<false>(c, tabs, i, 0u, 0, nullptr);
    r.exit = o.exit, r.nblk = o.nblk, r.mark = o.mark;
  }
  bool dirty = true;
  for (int round = 0; round < kGroup; ++round)
    if (!sync_round(c, tabs, i, valid, exits, &changed, r, dirty)) break;
  if (valid) a.rec[i] = r;
}

__global__ __launch_bounds__(kGroup) void jpeg_sync_chain_kernel(const SyncArgs a) {
  __shared__ js::Tabs tabs;
  __shared__ uint32_t exits[kGroup];
  __shared__ int changed;
  __shared__ int has[2][kGroup];
  __shared__ int val[2][kGroup];
  if ((*a.d.status & (kErrCount | kErrSequence)) != 0) return;
  const int tid = threadIdx.x;
  js::tabs_fill(tabs, a.d.tables, kJpegZigzag, tid, kGroup);
  __syncthreads();
  const js::Ctx c = make_ctx(a);
  uint32_t before = 0u;                   // the exit state of the subsequence in front of the group
  long long carry = 0;                    // the first block of the group's first subsequence
  for (int g = 0; g < a.groups; ++g) {
    const long long i = (long long)g * kGroup + tid;
    const bool valid = i < a.nsub;
    js::Rec r = {0u, 0u, 0u, -1};
    if (valid) r = a.rec[i];
    bool dirty = false;
    if (tid == 0) changed = 0;
    __syncthreads();
    if (tid == 0 && g > 0 && valid && before != r.entry) {
      r.entry = before;
      const js::Out o = js::decode_sub<false>(c, tabs, i, r.entry, 0, nullptr);
      r.exit = o.exit, r.nblk = o.nblk, r.mark = o.mark;
      dirty = true;
      changed = 1;
    }
    __syncthreads();
    const bool any = changed != 0;
    __syncthreads();
    if (any)
      for (int round = 0; round < kGroup; ++round)
        if (!sync_round(c, tabs, i, valid, exits, &changed, r, dirty)) break;
    if (valid && dirty) a.rec[i] = r;
    // the group's placement: an inclusive segmented scan of (holds a marker, blocks)
    int h = valid && r.mark >= 0 ? 1 : 0;
    long long v = valid ? (h ? js::interval_block0(c, (uint32_t)r.mark) : 0ll) + r.nblk : 0ll;
    int cur = 0;
    has[0][tid] = h, val[0][tid] = (int)(v < 0x7FFFFFFFll ? v : 0x7FFFFFFFll);
    exits[tid] = r.exit;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kGroup; d <<= 1) {
      int hh = has[cur][tid];
      long long vv = val[cur][tid];
      if (tid >= d && !hh) {
        hh = has[cur][tid - d];
        vv += val[cur][tid - d];
        vv = vv < 0x7FFFFFFFll ? vv : 0x7FFFFFFFll;
      }
      has[cur ^ 1][tid] = hh, val[cur ^ 1][tid] = (int)vv;
      cur ^= 1;
      __syncthreads();
    }
    long long first = carry;
    if (tid > 0) first = has[cur][tid - 1] ? (long long)val[cur][tid - 1] : carry + val[cur][tid - 1];
    first = first < 0x7FFFFFFFll ? first : 0x7FFFFFFFll;
    if (valid) a.blk0[i] = (int)first;
    carry = has[cur][kGroup - 1] ? (long long)val[cur][kGroup - 1] : carry + val[cur][kGroup - 1];
    carry = carry < 0x7FFFFFFFll ? carry : 0x7FFFFFFFll;
    before = exits[kGroup - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kGroup) void jpeg_sync_write_kernel(const SyncArgs a) {
  __shared__ js::Tabs tabs;
  if ((*a.d.status & (kErrCount | kErrSequence)) != 0) return;
  js::tabs_fill(tabs, a.d.tables, kJpegZigzag, threadIdx.x, kGroup);
  __syncthreads();
  const js::Ctx c = make_ctx(a);
  const long long i = (long long)blockIdx.x * kGroup + threadIdx.x;
  if (i >= a.nsub) return;
  const js::Out o = js::decode_sub<true>(c, tabs, i, a.rec[i].entry, (int64_t)a.blk0[i], a.d.coef);
  if (o.err) atomicOr(a.d.status, o.err);
}

// inclusive sums over the workgroup, through LDS; -> this thread's, and the workgroup's total
__device__ __forceinline__ int group_scan(int v, int (*buf)[kGroup], int& total) {
  const int tid = threadIdx.x;
  int cur = 0;
  buf[0][tid] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < kGroup; d <<= 1) {
    int x = buf[cur][tid];
    if (tid >= d) x = (int)((unsigned)x + (unsigned)buf[cur][tid - d]);
    buf[cur ^ 1][tid] = x;
    cur ^= 1;
    __syncthreads();
  }
  const int mine = buf[cur][tid];
  total = buf[cur][kGroup - 1];
  __syncthreads();
  return mine;
}

// NB: blocks per MCU, the first NY of them luma
template <int NB>
__global__ __launch_bounds__(kGroup) void jpeg_sync_dc_kernel(const SyncArgs a) {
  constexpr int NY = NB == 1 ? 1 : NB - 2, NC = NB - NY + 1;
  __shared__ int buf[2][kGroup];
  if ((*a.d.status & (kErrCount | kErrSequence)) != 0) return;
  const int nmcu = a.d.rows * a.d.cols;
  const long long m0 = (long long)blockIdx.x * a.d.ri;
  const long long m1 = m0 + a.d.ri < nmcu ? m0 + a.d.ri : nmcu;
  const int chunks = (int)((m1 - m0 + kGroup - 1) / kGroup);
  unsigned carry[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) carry[k] = 0u;
  for (int ch = 0; ch < chunks; ++ch) {
    const long long m = m0 + (long long)ch * kGroup + threadIdx.x;
    const bool valid = m < m1;
    short* blk = a.d.coef + (valid ? m : m0) * NB * 64;
    int d[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) d[b] = valid ? (int)blk[b * 64] : 0;
    unsigned sum[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) sum[k] = k ? (unsigned)d[NY + k - 1] : 0u;
#pragma unroll
    for (int b = 0; b < NY; ++b) sum[0] += (unsigned)d[b];
    unsigned base[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      int total;
      const int incl = group_scan((int)sum[k], buf, total);
      base[k] = carry[k] + (unsigned)incl - sum[k];
      carry[k] += (unsigned)total;
    }
    if (valid) {
      unsigned y = base[0];
#pragma unroll
      for (int b = 0; b < NY; ++b) {
        y += (unsigned)d[b];
        blk[b * 64] = (short)(unsigned short)(y & 0xFFFFu);
      }
#pragma unroll
      for (int k = 1; k < NC; ++k)
        blk[(NY + k - 1) * 64] = (short)(unsigned short)((base[k] + (unsigned)d[NY + k - 1]) & 0xFFFFu);
    }
  }
}

struct SyncLayout {
  DecLayout L;
  int64_t nsub, rec, blk0, bytes;
};

bool sync_layout(int h, int w, int samp, int64_t scan_bytes, int S, SyncLayout& Y) {
  if (S < 16 || S > 1024 || (S & (S - 1))) return false;
  if (!dec_layout(h, w, samp, scan_bytes, Y.L)) return false;
  Y.nsub = scan_bytes > 0 ? (scan_bytes + S - 1) / S : 1;
  int64_t at = Y.L.bytes;
  Y.rec = at, at += align256(Y.nsub * (int64_t)sizeof(js::Rec));
  Y.blk0 = at, at += align256(Y.nsub * 4);
  Y.bytes = at;
  return true;
}


// fn: the entry point's name, for its messages
int decode_rgb_sync(const char* fn, const unsigned char* scan, int64_t scan_bytes, int h, int w, int sampling,
                    int restart_interval, const unsigned char* qtables, const int32_t* tables, int y0, int y1,
                    int subseq_bytes, void* workspace, unsigned char* rgb, int64_t row_stride, int32_t* status,
                    void* stream) {
  VFML_REQUIRE(samp_ok(sampling), "%s: sampling %d (VFML_JPEG_420, _422, _444 or _GREY)", fn, sampling);
  VFML_REQUIRE(subseq_bytes >= 16 && subseq_bytes <= 1024 && (subseq_bytes & (subseq_bytes - 1)) == 0,
               "%s: subsequences of %d bytes (a power of two, 16..1024)", fn, subseq_bytes);
  SyncLayout Y;
  VFML_REQUIRE(sync_layout(h, w, sampling, scan_bytes, subseq_bytes, Y), "%s: picture %dx%d, scan of %lld "
               "bytes (sides of 1..65535, a scan below 2 GiB)", fn, w, h, (long long)scan_bytes);
  VFML_REQUIRE(scan && qtables && tables && workspace && rgb && status, "%s: null argument", fn);
  VFML_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, "%s: restart interval %d", fn, restart_interval);
  VFML_REQUIRE(0 <= y0 && y0 < y1 && y1 <= h, "%s: rows %d..%d of a picture of %d", fn, y0, y1, h);
  VFML_REQUIRE(row_stride >= (int64_t)3 * w, "%s: row stride %lld below the row's %d bytes", fn, (long long)row_stride,
               3 * w);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace must be 256-byte aligned", fn);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(tables) & 3u) == 0 && (reinterpret_cast<uintptr_t>(status) & 3u) == 0,
               "%s: tables and status must be 4-byte aligned", fn);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const DecLayout& L = Y.L;
  const int nmcu = L.rows * L.cols;
  SyncArgs sa;
  DecArgs& a = sa.d;
  // nothing of the scan can be skipped without markers: only the transform is windowed
  dec_args(a, L, ws, scan, scan_bytes, h, w, sampling, restart_interval, qtables, tables, y0, y1, rgb, row_stride, status);
  sa.rec = reinterpret_cast<js::Rec*>(ws + Y.rec);
  sa.blk0 = reinterpret_cast<int*>(ws + Y.blk0);
  sa.nsub = Y.nsub, sa.S = subseq_bytes;
  sa.groups = (int)((Y.nsub + kGroup - 1) / kGroup);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  dec_launch_markers(a, (unsigned)L.chunks, s);
  hipLaunchKernelGGL(jpeg_sync_group_kernel, dim3((unsigned)sa.groups), dim3(kGroup), 0, s, sa);
  hipLaunchKernelGGL(jpeg_sync_chain_kernel, dim3(1), dim3(kGroup), 0, s, sa);
  const hipError_t e = hipMemsetAsync(a.coef, 0, (size_t)nmcu * a.nb * 64 * sizeof(short), s);
  VFML_REQUIRE(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
  hipLaunchKernelGGL(jpeg_sync_write_kernel, dim3((unsigned)sa.groups), dim3(kGroup), 0, s, sa);
  const dim3 ints((unsigned)a.nint);
  switch (a.nb) {
    case 6: hipLaunchKernelGGL(jpeg_sync_dc_kernel<6>, ints, dim3(kGroup), 0, s, sa); break;
    case 4: hipLaunchKernelGGL(jpeg_sync_dc_kernel<4>, ints, dim3(kGroup), 0, s, sa); break;
    case 3: hipLaunchKernelGGL(jpeg_sync_dc_kernel<3>, ints, dim3(kGroup), 0, s, sa); break;
    default: hipLaunchKernelGGL(jpeg_sync_dc_kernel<1>, ints, dim3(kGroup), 0, s, sa); break;
  }
  dec_launch_picture(a, s);
  return vfml_check_launch(fn);
}

}  // namespace

extern "C" int64_t vfml_jpeg_decode_sync_sampled_workspace_bytes(int h, int w, int sampling, int64_t scan_bytes,
                                                                 int subseq_bytes) {
  SyncLayout Y;
  return sync_layout(h, w, sampling, scan_bytes, subseq_bytes, Y) ? Y.bytes : 0;
}

extern "C" int64_t vfml_jpeg_decode_sync_workspace_bytes(int h, int w, int64_t scan_bytes, int subseq_bytes) {
  return vfml_jpeg_decode_sync_sampled_workspace_bytes(h, w, kS420, scan_bytes, subseq_bytes);
}

extern "C" int vfml_jpeg_decode_rgb_sync_sampled(const unsigned char* scan, int64_t scan_bytes, int h, int w, int sampling,
                                                 int restart_interval, const unsigned char* qtables, const int32_t* tables,
                                                 int y0, int y1, int subseq_bytes, void* workspace, unsigned char* rgb,
                                                 int64_t row_stride, int32_t* status, void* stream) {
  return decode_rgb_sync("vfml_jpeg_decode_rgb_sync_sampled", scan, scan_bytes, h, w, sampling, restart_interval, qtables,
                         tables, y0, y1, subseq_bytes, workspace, rgb, row_stride, status, stream);
}

extern "C" int vfml_jpeg_decode_rgb_sync(const unsigned char* scan, int64_t scan_bytes, int h, int w, int restart_interval,
                                         const unsigned char* qtables, const int32_t* tables, int y0, int y1,
                                         int subseq_bytes, void* workspace, unsigned char* rgb, int64_t row_stride,
                                         int32_t* status, void* stream) {
  return decode_rgb_sync("vfml_jpeg_decode_rgb_sync", scan, scan_bytes, h, w, kS420, restart_interval, qtables, tables, y0,
                         y1, subseq_bytes, workspace, rgb, row_stride, status, stream);
}
