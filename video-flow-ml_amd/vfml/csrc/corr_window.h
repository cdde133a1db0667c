// Where a correlation lookup reads: the position of a texel in a tiled level image, a coordinate at a pyramid level and
// the origin of a query's window.  One definition for the lookups (flow_ops.hip) and for the pass that computes volume
// tiles on demand (corr_ensure.hip): the tiles that pass computes are exactly the ones these expressions make the lookup read.
#pragma once
#include "vfml_common.h"

namespace {

// Position of texel (y, x) of a w-wide image stored as (1<<tws) x (1<<ths) tiles, tile after tile, each tile row-major
// (tws = ths = 0: plain row-major).  A (2r+2)^2 lookup window then lies in ~8 128-byte lines instead of ~13 (ten 40-byte row
// segments): the lookup is bound by the lines it drags in, not by the texels it uses (tools/exp/lookup_tiled.py).
__device__ __forceinline__ int tiled_at(int y, int x, int w, int tws, int ths) {
  const int tpr = (w + (1 << tws) - 1) >> tws;
  return ((((y >> ths) * tpr + (x >> tws)) << (tws + ths)) + ((y & ((1 << ths) - 1)) << tws) + (x & ((1 << tws) - 1)));
}

// A level-0 coordinate at pyramid level l: c * 2^-l.  The factor is built from its exponent bits - exactly what
// 1.0f / (1 << l) is - so the product is exact and a compile-time level costs one multiply by a constant.
__device__ __forceinline__ float level_coord(float c, int l) {
  return c * __builtin_bit_cast(float, (127 - l) << 23);
}

// First integer-grid sample of a window along one axis: the (2r+2) samples origin .. origin + 2r + 1 around the level's
// coordinate c.  Clamped before the int conversion so that wild coordinates cannot overflow (NaN: far outside).
__device__ __forceinline__ int window_origin(float c, int radius) {
  return (int)fminf(fmaxf(floorf(c), -65536.f), 65536.f) - radius;
}

}  // namespace
