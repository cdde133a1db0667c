// ---- resident-A walk of the persistent GEMM form (SplitArgs::resident) ------------------------------
// Shared by conv_gemm_dma_kernel (conv_gemm_split.hip: the dense walk, a unit's column tiles are a contiguous run) and
// corr_ensure_kernel (corr_ensure.hip: a unit's column tiles are the set bits of a mask).  One body, gemm_resident_unit.
//
// The correlation GEMMs have a short K axis (256 channels = four 64-channel steps of hi halves) and a very wide output:
// a tile's stores are the work, and the streaming walk opens every K step with a wait on a fresh L2 -> LDS round
// trip that queues behind those stores (measured ~1 us per step and tile).  Here a workgroup (four waves, 80 KB of LDS,
// two per CU as there) keeps its operands whole:
//  * the 128-row tile of the activation operand, all its K steps (64 KB), is staged ONCE per work unit - a unit is one
//    row tile x a list of 64-column tiles; each wave owns 32 rows x 64 columns and takes its rows'
//    fragments out of the image into 64 registers, where they stay for every column tile of the unit;
//  * the weight operand comes a whole column tile at a time (all K steps, 32 KB) into one of two buffers: tile j + 1 is
//    requested when tile j starts, so a tile waits ONCE, for operands requested a whole tile earlier;
//  * each wave has a private 4 KB transposition slab that aliases no operand (a 32 x 32 block at a time).
// vmcnt accounting, in a wave's issue order: [B(j)] [stores(j-1)] at the top of tile j - the counted wait leaves
// exactly the stores outstanding (8 per wave, 16 with the twin: every store instruction is issued, out-of-range lanes
// carry an out-of-range offset), so it waits for B(j) and never for a store younger than it; then [B(j+1)] goes out
// behind the barrier.  Only a unit's start waits vmcnt(0): for its A image, then for B(0) (the youngest operations).
// The barriers wait for LDS only (lds_barrier): __syncthreads() would drain the DMAs in flight.
// Same LDS image, fragment addresses, MFMA operands and K order, and the same epilogue expressions as the streaming
// walk: the outputs are bit-identical to it.
#pragma once
#include "conv_split_common.h"

namespace {

// The column tiles of a dense unit: the run nt0 .. nt1 - 1.  (What gemm_resident_unit asks of its list: first(), the
// first tile or -1; next(nt), the tile after nt or -1 - both uniform over the workgroup.)
struct ResidentRun {
  int nt0, nt1;
  __device__ __forceinline__ int first() const { return nt0 < nt1 ? nt0 : -1; }
  __device__ __forceinline__ int next(int nt) const { return nt + 1 < nt1 ? nt + 1 : -1; }
};

// One work unit: row tile mt against the column tiles of `cols`, in the list's order.
template <bool H16, bool BIAS, class Cols>
__device__ __forceinline__ void gemm_resident_unit(const SplitArgs& a, char* smem, int mt, const Cols& cols) {
  constexpr int NW = 4;
  constexpr int RBM = 128, RBN = 64;                       // workgroup tile
  constexpr int NSTEP = VFML_RESIDENT_KMAX / 64;           // K steps the images hold
  constexpr int ASTEP = RBM * 128, BSTEP = RBN * 128;      // one step's image: rows x 128 B (64 hi halves)
  // LDS: two B buffers (the A image of a unit passes through the same 64 KB on its way to registers), then the slabs
  constexpr int BOFF = 0, BBUF = NSTEP * BSTEP, SLAB = BOFF + 2 * BBUF;
  constexpr int AP = RBM / (8 * NW), BP = RBN / (8 * NW);  // 1-KiB pieces (8 rows x 128 B) per wave per step
  constexpr int ES = H16 ? 2 : 4;
  constexpr int NSTORE = 8, NSTORE_T = 16;                 // store instructions per wave and tile (with the twin)
  constexpr int STORE_NT = 2;
  static_assert(NSTEP * ASTEP == 2 * BBUF, "the A image of a unit fills the two B buffers");
  static_assert(SLAB + NW * 32 * 32 * 4 == VFML_RESIDENT_LDS, "LDS budget of the resident-A walk: two workgroups per CU");

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  // loader: as the streaming walk (piece j of a wave = tile rows 32 j + 8 wave .. + 7, source-side swizzle)
  const int lrow = 8 * wave + (lane >> 3);
  const int piece = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);
  const int nk = (a.Kp / 64 + 1) & ~1;                     // rounded up to even by an all-zero step, as there
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.wbase), 0, a.bytesb, 0x00020000);
  // fragments: wave = row block, both 32-column blocks
  const int r = lane & 31, half = lane >> 5;
  const int q16 = (((r >> 1) & 7) ^ half) * 16;
  const int aoff = (wave * 32 + r) * 128 + q16;
  const int boff = r * 128 + q16;
  float* ws = reinterpret_cast<float*>(smem + SLAB) + wave * (32 * 32);   // one 32 x 32 block at a time
  const int c4 = (lane % 8) * 4, rr = lane / 8;            // epilogue: slab row rr of eight, columns c4 .. + 3

  const int m0 = mt * RBM;
  const int rows_valid = a.M - m0 < RBM ? a.M - m0 : RBM;
  __amdgpu_buffer_rsrc_t r0;
  if (a.tilebase)
    r0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in0) + (int64_t)m0 * a.ld0, 0,
                                           ((rows_valid - 1) * a.ld0 + a.d0off + a.c0) * 4, 0x00020000);
  else
    r0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in0), 0, a.bytes0, 0x00020000);
  int va[AP];
#pragma unroll
  for (int j = 0; j < AP; ++j) {
    const int m = m0 + 8 * NW * j + lrow;
    const int mrow = a.tilebase ? m - m0 : m;
    va[j] = m < a.M ? (mrow * a.ld0 + a.d0off) * 4 + piece * 32 : OOB;
  }
  auto issue_b = [&](int nt, int buf) {
    int colbase[BP];
#pragma unroll
    for (int j = 0; j < BP; ++j) {
      const int col = nt * RBN + 8 * NW * j + lrow;
      colbase[j] = col < a.cout ? a.whi_off + col * a.Kp * 2 + piece * 16 : (a.bhi ? 0x7ffffff0 : 0x40000000);
    }
    for (int s = 0; s < nk; ++s)
#pragma unroll
      for (int j = 0; j < BP; ++j)
        dma16(rb, colbase[j], s * 128, smem + BOFF + buf * BBUF + s * BSTEP + wave * (8 * 128) + j * (8 * NW * 128));
  };

  // The unit's A image passes through the two B buffers; each wave pulls its own fragments (32 rows, all K steps: 64
  // VGPRs) out of it and keeps them for the whole unit, so a tile reads only B fragments from LDS.
  h16x8 af[4 * NSTEP];
#pragma unroll
  for (int q = 0; q < 4 * NSTEP; ++q) af[q] = h16x8{0, 0, 0, 0, 0, 0, 0, 0};
  lds_barrier();                           // every wave is done with the previous unit's B buffers
  for (int s = 0; s < nk; ++s) {
    const bool past = s * 64 >= a.ctot;    // the rounding-up step of an odd step count: zeros
#pragma unroll
    for (int j = 0; j < AP; ++j)
      dma16(r0, past ? OOB : va[j], s * 256, smem + s * ASTEP + wave * (8 * 128) + j * (8 * NW * 128));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (once per unit: also the previous unit's last stores)
  lds_barrier();                           // the A image landed for every wave
  static_for<NSTEP>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    if (s < nk) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) af[s * 4 + ks] = *reinterpret_cast<const h16x8*>(smem + s * ASTEP + (aoff ^ (ks * 32)));
    }
  });
  lds_barrier();                           // every wave has its fragments (lgkmcnt(0)): the buffers are B's again
  int nt = cols.first();
  if (nt >= 0) issue_b(nt, 0);

  for (int i = 0; nt >= 0; ++i) {
    const int buf = i & 1;
    const int nxt = cols.next(nt);
    const int n0 = nt * RBN;
    if (i == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (a.out_t) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSTORE_T) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSTORE) : "memory");
    lds_barrier();                         // B(nt) landed for every wave; the other buffer's readers are done
    f32x4 bv[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if constexpr (BIAS) {                  // (before the next tile's DMAs: its wait then leaves them in flight)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (n0 + j * 32 + c4 < a.cout) bv[j] = *reinterpret_cast<const f32x4*>(a.bias + n0 + j * 32 + c4);
    }
    if (nxt >= 0) issue_b(nxt, buf ^ 1);

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    // K steps in pairs (the step count is even): each pair is one straight-line block, so the fragment reads of
    // the whole pair can go out ahead of its MFMAs
    const char* bb = smem + BOFF + buf * BBUF;
    static_for<NSTEP / 2>([&](auto pc) {
      constexpr int s0 = 2 * decltype(pc)::value;
      if (s0 < nk) {
        h16x8 b0[8], b1[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          b0[q] = *reinterpret_cast<const h16x8*>(bb + (s0 + (q >> 2)) * BSTEP + (boff ^ ((q & 3) * 32)));
          b1[q] = *reinterpret_cast<const h16x8*>(bb + (s0 + (q >> 2)) * BSTEP + (boff ^ ((q & 3) * 32)) + 4096);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[s0 * 4 + q], b0[q], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[s0 * 4 + q], b1[q], acc[1], 0, 0, 0);
        }
      }
    });

    // epilogue: the streaming walk's direct one, one 32 x 32 block of the wave at a time through its 4 KB slab: a
    // store instruction covers 8 rows x 128 contiguous bytes (of out, and of out_t)
    const int cols_valid = a.cout - n0 < RBN ? a.cout - n0 : RBN;
    char* tbase = reinterpret_cast<char*>(a.out) + ((int64_t)m0 * a.ldo + n0) * ES;
    const __amdgpu_buffer_rsrc_t ro =
        __builtin_amdgcn_make_buffer_rsrc(tbase, 0, ((rows_valid - 1) * a.ldo + cols_valid) * ES, 0x00020000);
    const int rows_t = cols_valid, cols_t = rows_valid;        // extent of the transposed tile
    __amdgpu_buffer_rsrc_t rt = ro;
    if (a.out_t) {
      char* tbase_t = reinterpret_cast<char*>(a.out_t) + ((int64_t)n0 * a.ld_out_t + m0) * ES;
      rt = __builtin_amdgcn_make_buffer_rsrc(tbase_t, 0, ((rows_t - 1) * a.ld_out_t + cols_t) * ES, 0x00020000);
    }
    static_for<2>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      const int gcol = j * 32 + c4;                            // column within the tile
#pragma unroll
      for (int e = 0; e < 16; ++e) ws[((e & 3) + 8 * (e >> 2) + 4 * half) * 32 + r] = acc[j][e];
      // (same wave, LDS operations complete in order: no barrier between the writes and the reads)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        f32x4 v = *reinterpret_cast<const f32x4*>(ws + (p * 8 + rr) * 32 + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = (v[e] * a.w_inv + bv[j][e]) * a.out_scale;   // same expression as epilogue_rows
          if (a.epilogue == VFML_EPI_RELU) v[e] = fmaxf(v[e], 0.f);
        }
        const int off = gcol < cols_valid ? ((wave * 32 + p * 8 + rr) * a.ldo + gcol) * ES : OOB;
        if constexpr (H16) {
          const h16x2 p0 = {(_Float16)v[0], (_Float16)v[1]}, p1 = {(_Float16)v[2], (_Float16)v[3]};
          const u32x2 hv = {__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1)};
          __builtin_amdgcn_raw_buffer_store_b64(hv, ro, off, 0, STORE_NT);
        } else {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ro, off, 0, STORE_NT);
        }
      }
      if (a.out_t) {
        // the transposed copy, out_t[column][row]: the block through the same slab as [column][row], row index
        // rotated by column >> 1
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = (e & 3) + 8 * (e >> 2) + 4 * half;
          ws[r * 32 + ((row + (r >> 1)) & 31)] = acc[j][e];
        }
        const int g = lane >> 3, cl = lane & 7;
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {
          const int c = pp * 8 + cl;                            // column of the block
          f32x4 v;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = ws[c * 32 + ((4 * g + k + (c >> 1)) & 31)] * a.w_inv * a.out_scale;
          const int trow = j * 32 + c;                          // column of the tile = row of out_t
          const int q0 = wave * 32 + 4 * g;                     // first of the four pixels (columns of out_t)
          const bool ok = trow < rows_t && q0 < cols_t;         // M % 4 == 0 (host check): a quad is whole
          if constexpr (H16) {
            const h16x2 p0 = {(_Float16)v[0], (_Float16)v[1]}, p1 = {(_Float16)v[2], (_Float16)v[3]};
            const u32x2 hv = {__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1)};
            __builtin_amdgcn_raw_buffer_store_b64(hv, rt, ok ? (trow * a.ld_out_t + q0) * 2 : OOB, 0, STORE_NT);
          } else {
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rt, ok ? (trow * a.ld_out_t + q0) * 4 : OOB, 0, STORE_NT);
          }
        }
      }
    });
    nt = nxt;
  }
}

// The dense walk.  Units are numbered column-run-major (u = run * mtiles + row tile) and dealt round-robin, so the
// workgroups in flight walk the same columns of different row tiles: a weight tile pulled into an XCD's L2 serves every
// workgroup there.
template <bool H16, bool BIAS>
__device__ __forceinline__ void gemm_resident_walk(const SplitArgs& a, char* smem) {
  const int units = a.mtiles * a.res_nc;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int run = u / a.mtiles, mt = u - run * a.mtiles;
    const int nt0 = run * a.res_cl;
    const int nt1 = nt0 + a.res_cl < a.ntiles ? nt0 + a.res_cl : a.ntiles;
    gemm_resident_unit<H16, BIAS>(a, smem, mt, ResidentRun{nt0, nt1});
  }
}

}  // namespace
