// Levels of a correlation pyramid on demand (vfml_corr_levels_ensure; vfml_corr_level0_ensure is its one-level call): in
// front of a lookup, compute exactly the 128 x 64 tiles of the f32 volumes that the lookup's windows are about to read and
// that are not there yet.
//
// A lookup reads a (2r+2)^2 window per query and level; a row of the 1080p level-0 volume has 32640 columns, of level 1
// 8640, of level 2 2400.  With spatially coherent flow the windows of the 128 queries of a row tile (a 16 x 8 block of
// cells in 4 x 8 tile order) fall into a few of a level's column tiles (2 % of level 0's, 6 % of level 1's, 16 % of level
// 2's), so the dense GEMMs of a frame pair store mostly values that nothing ever reads.  Here a pair's on-demand levels
// start empty, each with a bitmap (one bit per row tile x column tile, in HBM) of what has been computed:
//   work unit  (centre frame, direction, row tile of 128 volume rows), dealt round-robin over a persistent grid of two
//              workgroups per CU; exactly one workgroup owns a row tile of a pyramid in a launch
//   1          the unit's 128 queries -> their coordinates, read once (the row -> (y, x) map is the inverse of the tile
//              order of the level-0 map, whatever levels are asked for)
//   then, for every requested level in ascending order:
//   2          the column tiles the queries' windows touch at that level, as a bit mask in LDS - the level coordinate, the
//              window origin and the texel position are the lookup's own expressions (corr_window.h); a texel outside the
//              level image is zeroed by the lookup whatever it loaded from its clamped address, so it asks for no tile.  A
//              texel inside the image lies below the level's column count, so no bit at or beyond its tile count is set
//              even where the last tile is ragged (2400 columns: 37.5 tiles)
//   3          minus the tiles the level's bitmap has
//   4          nothing left: next level
//   5          else the resident-A walk's unit (gemm_resident_walk.h: A image staged, B a column tile at a time and one
//              ahead, the counted vmcnt, the slab stores) with that level's arguments over the set bits of the mask instead
//              of a contiguous run; its own column bound cuts a ragged last tile, as in the dense call
//   6, 7       the stores are waited for by every wave, then the tiles' bits are set
// All levels of a unit in ONE launch: a launch that only checks costs 8.6 us, and one per level in front of each of a
// field's twelve lookups would give back a third of what the pooled levels' dense GEMMs cost.  The A image (the query
// rows) is the same for every level of a unit; it is staged again by each level that computes tiles.
// Same operands, same MFMA sequence, K order and epilogue expression as the dense call of the level: the values are the
// ones the dense GEMM writes (and, one MFMA per product being symmetric in its operands, the ones its transposed twin
// writes).  The operands are reached through device cells (vfml_ptr_table_set), so one captured launch serves every window.
#include "gemm_resident_walk.h"
#include "corr_window.h"

namespace {

constexpr int ENSURE_MASK_WORDS = 64;      // column tiles of a volume row: at most 2048, one mask word per lane of a wave
constexpr int ENSURE_MAX_LEVELS = 3;       // levels of one launch (the f32 levels of a pyramid that are worth it)

struct EnsureLevel {
  SplitArgs g;                 // the level's dense call; in0 / wbase / out come from the unit's cells
  int h, w;                    // the level image
  int wpr;                     // bitmap words per row tile
  int level;                   // coordinates are scaled by 2^-level; the level's counter cell
};

struct EnsureArgs {
  EnsureLevel lv[ENSURE_MAX_LEVELS];
  int nlev;
  const void* const* cells;    // per (direction, centre): query rows, then per level target hi plane, level buffer, bitmap
  const float* coords;
  unsigned* counter;           // tiles computed, cell `level`, added per unit and level that computes any (or null)
  int ld_coords, dir_coords;
  int centres, dirs, dir_cells;
  int q_per_map;
  int h, w, radius, tws, ths;  // the query map (= the level-0 image): the rows' order
};
static_assert(sizeof(EnsureArgs) <= 4096, "the levels' arguments travel as kernel arguments");

// A unit's column tiles: the set bits of its mask in ascending order.  Lane w of every wave holds word w.
struct MaskCols {
  unsigned v;
  int nw;
  __device__ __forceinline__ unsigned word(int w) const {
    return (unsigned)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(w));
  }
  __device__ __forceinline__ int from(int at) const {      // first tile >= at, or -1 (at: uniform)
    int w = at >> 5;
    if (w >= nw) return -1;
    unsigned m = word(w) & (~0u << (at & 31));
    while (!m) {
      if (++w >= nw) return -1;
      m = word(w);
    }
    return w * 32 + __builtin_ctz(m);
  }
  __device__ __forceinline__ int first() const { return from(0); }
  __device__ __forceinline__ int next(int nt) const { return from(nt + 1); }
};

// A pointer read from a device cell, as ONE value per wave: the load is a vector load, and without this every buffer
// descriptor built from the pointer is taken for divergent - each LDS-DMA and store of the walk then sits in a waterfall
// loop (readfirstlane, compare, saveexec, branch) that the dense walk, whose pointers are kernel arguments, does not have.
__device__ __forceinline__ const void* uniform_cell(const void* const* cell) {
  const uint64_t v = reinterpret_cast<uint64_t>(*cell);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return reinterpret_cast<const void*>(((uint64_t)hi << 32) | lo);
}

typedef __attribute__((address_space(1))) unsigned* gu32ptr;
typedef const __attribute__((address_space(1))) float* gf32cptr;

typedef const __attribute__((address_space(4))) EnsureArgs* ensure_kargs_t;

// The arguments are read through the kernel-argument segment itself (EnsureArgs is the kernel's one argument, at its
// start), and every work unit reads what it needs anew: as plain by-value arguments the compiler loads all of them once,
// ahead of the unit loop, and keeps them in scalar registers across the walk, which has none to spare - with three
// levels' arguments that ended in a stack frame (tests/test_abi.py: no kernel of the library has one).
__global__ __launch_bounds__(256, 2) void corr_ensure_kernel(const EnsureArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* mask = reinterpret_cast<unsigned*>(smem);      // (aliases the walk's operand buffers: barriers below)
  const int t = threadIdx.x, lane = t & 63;
  const ensure_kargs_t kargs = (ensure_kargs_t)__builtin_amdgcn_kernarg_segment_ptr();
  const int mtiles = kargs->lv[0].g.mtiles;                // (every level has the queries' rows)
  const int units = kargs->centres * kargs->dirs * mtiles;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    ensure_kargs_t fresh = kargs;
    asm volatile("" : "+s"(fresh));                        // (nothing read through it is carried over from the last unit)
    const EnsureArgs& e = *(const EnsureArgs*)fresh;
    const int tsh = e.tws + e.ths;
    const int tpr = (e.w + (1 << e.tws) - 1) >> e.tws;
    const int side = 2 * e.radius + 2;
    const int ucells = 1 + 3 * e.nlev;
    const int k = u / mtiles, mt = u - k * mtiles;
    const int dir = k / e.centres, c = k - dir * e.centres;
    const void* const* cell = e.cells + (dir * e.dir_cells + c) * ucells;
    // volume row -> query: the inverse of tiled_at on the query map; its level-0 coordinate serves every level
    bool live = false;
    float cx = 0.f, cy = 0.f;
    if (t < 128) {
      const int row = mt * 128 + t;
      const int tile = row >> tsh, in = row & ((1 << tsh) - 1);
      const int ty = tile / tpr, tx = tile - ty * tpr;
      const int y = (ty << e.ths) + (in >> e.tws), x = (tx << e.tws) + (in & ((1 << e.tws) - 1));
      if (row < e.lv[0].g.M && y < e.h && x < e.w) {
        const gf32cptr cr = (gf32cptr)e.coords + ((int64_t)c * e.q_per_map + y * e.w + x) * e.ld_coords + dir * e.dir_coords;
        live = true;
        cx = cr[0];
        cy = cr[1];
      }
    }
    for (int i = 0; i < e.nlev; ++i) {
      const EnsureLevel& lv = e.lv[i];
      const int wpr = lv.wpr;
      const gu32ptr bitmap = (gu32ptr)uniform_cell(cell + 3 + 3 * i) + mt * wpr;
      lds_barrier();                           // every wave is done with the previous level's (or unit's) buffers
      if (t < ENSURE_MASK_WORDS) mask[t] = 0u;
      lds_barrier();
      if (live) {
        const int x0 = window_origin(level_coord(cx, lv.level), e.radius);
        const int y0 = window_origin(level_coord(cy, lv.level), e.radius);
        const int xlo = max(x0, 0), xhi = min(x0 + side - 1, lv.w - 1);
        const int ylo = max(y0, 0), yhi = min(y0 + side - 1, lv.h - 1);
        if (xlo <= xhi && ylo <= yhi) {
          for (int yy = ylo; yy <= yhi; yy = ((yy >> e.ths) + 1) << e.ths)
            for (int xx = xlo; xx <= xhi; xx = ((xx >> e.tws) + 1) << e.tws) {
              const int ct = tiled_at(yy, xx, lv.w, e.tws, e.ths) >> 6;     // the 64-column tile of that texel
              atomicOr(&mask[ct >> 5], 1u << (ct & 31));
            }
        }
      }
      lds_barrier();
      // minus what the pair's bitmap has: ONE wave reads it, so that every wave walks the same list whatever a second
      // unit of the same pyramid (a window that repeats a frame) sets meanwhile
      if (t < wpr) mask[t] &= ~bitmap[t];
      lds_barrier();
      const unsigned need = lane < wpr ? mask[lane] : 0u;
      const MaskCols cols{need, wpr};
      int cnt = 0;
      for (int w = 0; w < wpr; ++w) cnt += __builtin_popcount(cols.word(w));
      if (cnt == 0) continue;

      SplitArgs a = lv.g;
      a.in0 = a.in1 = reinterpret_cast<const float*>(uniform_cell(cell));
      a.wbase = reinterpret_cast<const char*>(uniform_cell(cell + 1 + 3 * i));
      a.out = reinterpret_cast<float*>(const_cast<void*>(uniform_cell(cell + 2 + 3 * i)));
      gemm_resident_unit<false, false>(a, smem, mt, cols);    // (opens with a barrier: every wave has read its mask word)

      // (the lookup is a later launch: tiles and bits reach it with this kernel's end, like any kernel's output - no
      // cache write-back is asked for here; the wait only keeps a bit from being set ahead of its tile)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this wave's tile stores are complete ...
      lds_barrier();                                           // ... and every wave's: the tiles are there
      if (t < wpr && need) atomicOr((unsigned*)bitmap + t, need);
      if (t == 0 && e.counter) atomicAdd(e.counter + lv.level, (unsigned)cnt);
    }
  }
}

// What both entry points do: nlev levels in ascending order, every check, the launch.
int ensure_levels(const char* who, const vfml_corr_level_desc* lv, int nlev, int in_fmt, int k_order, const void* const* cells,
                  int centres, int dirs, int dir_cells, const float* coords, int ld_coords, int dir_coords, int h, int w,
                  int radius, int vol_tile, uint32_t* counter, void* stream) {
  VFML_REQUIRE(nlev >= 1 && nlev <= ENSURE_MAX_LEVELS, "%s: one to %d levels", who, ENSURE_MAX_LEVELS);
  EnsureArgs e;
  e.tws = vol_tile & 15;
  e.ths = vol_tile >> 4;
  VFML_REQUIRE(vol_tile >= 0 && e.ths <= 6 && e.tws + e.ths <= 6, "%s: vol_tile: tiles of at most 64 texels", who);
  VFML_REQUIRE(h > 0 && w > 0 && radius >= 1 && radius <= 4, "%s: empty level image, or radius outside 1..4", who);
  const auto tiled_count = [&](int hh, int ww) {
    return (int64_t)(((hh - 1) >> e.ths) + 1) * (((ww - 1) >> e.tws) + 1) << (e.tws + e.ths);
  };
  const int64_t rows = tiled_count(h, w);
  for (int i = 0; i < nlev; ++i) {
    EnsureLevel& l = e.lv[i];
    VFML_REQUIRE(lv[i].d, "%s: null desc / cells / coords", who);
    if (const int rc = vfml_detail::prepare_resident_gemm(lv[i].d, lv[i].w_hi, lv[i].w_lo, lv[i].kp, lv[i].w_scale, in_fmt,
                                                          lv[i].out_fmt, k_order, who, &l.g))
      return rc;
    const SplitArgs& a = l.g;
    VFML_REQUIRE(!a.bias && !a.out_t && a.epilogue == VFML_EPI_NONE && a.whi_off == 0 && a.d0off == 0 && a.tilebase,
                 "%s: the level-0 call has no bias, twin or activation, its hi plane leads its planes and its rows are one "
                 "split-row source", who);
    VFML_REQUIRE(lv[i].level >= 0 && lv[i].level <= 7 && (i == 0 || lv[i].level > lv[i - 1].level) && lv[i].h > 0 && lv[i].w > 0,
                 "%s: levels 0..7 in ascending order, no empty level image", who);
    const int64_t tiled = tiled_count(lv[i].h, lv[i].w);
    VFML_REQUIRE(rows == a.M, "%s: the call's rows (%d) must be the %lld positions of the tiled %d x %d query map", who, a.M,
                 (long long)rows, h, w);
    VFML_REQUIRE(tiled == a.cout, "%s: the call's columns (%d) must be the %lld positions of the tiled %d x %d level image", who,
                 a.cout, (long long)tiled, lv[i].h, lv[i].w);
    VFML_REQUIRE(i == 0 || (a.c0 == e.lv[0].g.c0 && a.ld0 == e.lv[0].g.ld0 && a.Kp == e.lv[0].g.Kp),
                 "%s: every level's call has the same query rows", who);
    l.h = lv[i].h; l.w = lv[i].w; l.level = lv[i].level;
    l.wpr = (a.ntiles + 31) / 32;
    VFML_REQUIRE(l.wpr <= ENSURE_MASK_WORDS, "%s: at most %d column tiles per volume row", who, ENSURE_MASK_WORDS * 32);
  }
  VFML_REQUIRE(centres >= 1 && (dirs == 1 || dirs == 2) && dir_cells >= (dirs == 2 ? centres : 0) && ld_coords >= 2 &&
               dir_coords >= 0, "%s: centres >= 1, one or two directions, the second direction's cells behind the first's", who);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(cells) & 7u) == 0 && (!counter || (reinterpret_cast<uintptr_t>(counter) & 3u) == 0),
               "%s: cells are 8-byte aligned, the counter 4-byte", who);
  for (int i = nlev; i < ENSURE_MAX_LEVELS; ++i) e.lv[i] = e.lv[0];      // (never read: no uninitialised bytes in the arguments)
  e.nlev = nlev;
  e.cells = cells; e.coords = coords; e.counter = counter;
  e.ld_coords = ld_coords; e.dir_coords = dir_coords;
  e.centres = centres; e.dirs = dirs; e.dir_cells = dir_cells;
  e.q_per_map = h * w; e.h = h; e.w = w; e.radius = radius;
  if (const int rc = vfml_lds_cap(reinterpret_cast<const void*>(&corr_ensure_kernel), VFML_RESIDENT_LDS, who)) return rc;
  const int64_t units = (int64_t)centres * dirs * e.lv[0].g.mtiles;
  hipLaunchKernelGGL(corr_ensure_kernel, dim3((int)(units > 512 ? 512 : units)), dim3(256), VFML_RESIDENT_LDS,
                     reinterpret_cast<hipStream_t>(stream), e);
  return vfml_check_launch(who);
}

}  // namespace

extern "C" int vfml_corr_levels_ensure(const vfml_corr_level_desc* levels, int nlevels, int in_fmt, int k_order,
                                       const void* const* cells, int centres, int dirs, int dir_cells, const float* coords,
                                       int ld_coords, int dir_coords, int h, int w, int radius, int vol_tile,
                                       uint32_t* counters, void* stream) {
  const char* who = "vfml_corr_levels_ensure";
  VFML_REQUIRE(levels && cells && coords, "%s: null levels / cells / coords", who);
  return ensure_levels(who, levels, nlevels, in_fmt, k_order, cells, centres, dirs, dir_cells, coords, ld_coords, dir_coords,
                       h, w, radius, vol_tile, counters, stream);
}

extern "C" int vfml_corr_level0_ensure(const vfml_conv_desc* d, const void* w_hi, const void* w_lo, int kp, float w_scale,
                                       int in_fmt, int out_fmt, int k_order, const void* const* cells, int centres, int dirs,
                                       int dir_cells, const float* coords, int ld_coords, int dir_coords, int h, int w,
                                       int radius, int vol_tile, uint32_t* counter, void* stream) {
  const char* who = "vfml_corr_level0_ensure";
  VFML_REQUIRE(d && cells && coords, "%s: null desc / cells / coords", who);
  const vfml_corr_level_desc lv = {d, w_hi, w_lo, kp, w_scale, out_fmt, 0, h, w};
  return ensure_levels(who, &lv, 1, in_fmt, k_order, cells, centres, dirs, dir_cells, coords, ld_coords, dir_coords, h, w,
                       radius, vol_tile, counter, stream);
}
