// How a vfml_conv2d_split call becomes a kernel: plan_split() below is the whole decision, read top to bottom.
//
// vfml_conv2d_split (conv_gemm_split.hip) runs three steps: it validates the descriptor and fills SplitArgs, asks
// plan_split which template instantiation runs the call, and looks that plan up in the family's table of the
// instantiations that exist (a plan without a row is an error).  vfml_conv2d_split_variant stops after the look-up and
// prints the row's name.  plan_split is pure host code: no HIP call, no pointer dereferenced, no environment read.
#include <stdio.h>
#include "conv_split_common.h"

namespace vfml_detail {

namespace {

// Register-staged kernel, cout > 64: 128 columns per workgroup unless 64-wide tiles use the machine better.  Efficiency
// model = (useful columns / padded columns) x (workgroups / slots of the last partial round) x a 0.7 handicap for the
// narrower tile (half the MFMAs per loaded A element; measured: 64-wide tiles lose more than the tail round gains on the
// 1080p shapes); 2 workgroups per CU.
double reg_eff(const SplitArgs& a, int w) {
  const int nt = (a.cout + w - 1) / w;
  const int64_t wg = (int64_t)a.mtiles * nt, slots = 512;     // (a.mtiles: row tiles of BM = 128 pixels)
  const int64_t rounds = (wg + slots - 1) / slots;
  return ((double)a.cout / (nt * w)) * ((double)wg / (rounds * slots)) * (w == 64 ? 0.7 : 1.0);
}

// LDS-DMA kernel, cout > 64: 192 x 128, 128 x 192, 128 x 128 or 128 x 64 tiles (two workgroups per CU each).  Cost model:
// (rounds over the 512 resident slots; a problem that does not fill them is one round, a longer one costs its
// fractional number of rounds because workgroups of the last round run less contended) x (MFMAs per tile / measured
// relative efficiency of the tile shape: fewer operand bytes per MFMA on the larger tiles).
// (the 8-wave shapes of round 1 - 256 x 128, 192 x 256, 256 x 256, one workgroup per CU - measured slower and are no
// longer built)
double dma_cost(const SplitArgs& a, int tbm, int tbn, double mf, double eff) {
  const double tiles = (double)((a.M + tbm - 1) / tbm) * (double)((a.cout + tbn - 1) / tbn);
  return (tiles > 512.0 ? tiles / 512.0 : 1.0) * mf / eff;
}

// The tile shape (TM TN WM WN as digits) the shared-stage kernel (conv_gemm_tapx.hip) would run the call on, or 0 when
// the call is not its: stride-1 "same" convolutions over split-row sources on the uniform-step loader, 2..5 taps per
// filter row, three MFMAs per product or one over 64-channel steps.  `cfg` = the shape chosen among the per-tap ones.
int tapx_cfg(const SplitArgs& a, int cfg, bool forced) {
  if (!(a.fastk && !a.direct && !a.pointwise && !a.tilebase && a.stride == 1 && a.ho == a.H && a.wo == a.W && a.kw >= 2 &&
        a.kw <= VFML_TAPX_KWMAX && a.kh <= 4 && (a.nm == 3 || a.nm == 5)))
    return 0;
  if (a.cout <= 32) return 0;
  if (forced) return (cfg == 3222 || cfg == 2322 || (cfg == 2241 && a.cout <= 64) || (cfg == 2341 && a.cout <= 96)) ? cfg : 0;   // (VFML_DMA_TILE)
  if (a.cout <= 96) {
    // 256 x 64 / 256 x 96 tiles, when they fill the 512 resident slots of their last round to 85 % (the 1080p 1/8-scale
    // maps are 380 such tiles: three quarters of one round - the per-tap kernel's 128-row tiles serve those better)
    const int64_t tiles = (a.M + 255) / 256, rounds = (tiles + 511) / 512;
    if (tiles * 100 < rounds * 512 * 85) return 0;
    return a.cout <= 64 ? 2241 : 2341;
  }
  return cfg == 3222 || cfg == 2322 ? cfg : 0;
}

}  // namespace

int plan_split(const SplitArgs& a, bool in16, int flags, int forced_tile, SplitPlan* plan) {
  // fp32 NHWC sources: the register-staged kernel, 128 pixels x BN channels
  if (!in16) {
    int bn = a.cout > 64 ? 128 : (a.cout > 32 ? 64 : 32);
    if (a.cout > 64 && reg_eff(a, 64) > reg_eff(a, 128)) bn = 64;
    *plan = reg_plan(bn, bn == 32 ? 4 : 2, bn == 32 ? 1 : 2, a.ctot >= BK, false, a.nm);
    return 0;
  }

  // Split-row sources: the LDS-DMA kernels.  The GEMM form (plain output straight from the accumulators) is one
  // persistent tile shape, 128 x 128: the one that does not spill.
  // It stays on 32x32x16 MFMAs: measured with 16x16x32 (an experiment since removed) the 32400^2 volume gains 4 %, the
  // MemFlow read-out 2 %, the 1080p field nothing - and v_mfma_f32_16x16x32_f16 is NOT symmetric in its operands to the
  // last bit (a volume stored transposed and the reverse problem computed directly differ in the last ulp, which the
  // 32x32x16 form never does: tests/test_gpu_kernels.py::test_wide_gemm_with_transposed_second_output), so the
  // sliding job's "volume + transposed volume from one pass" would stop being bit-identical to from-scratch fields.
  if (a.direct) {
    // (the validation has made sure that VFML_FMT_F16 outputs, VFML_CONV_SWAP_CROSS and single-plane weights come with
    // the uniform-step loader, and VFML_CONV_SWAP_CROSS with the full product)
    VFML_REQUIRE(a.fastk || !(a.nm == 2 && a.bhi), "vfml_conv2d_split: a weight operand without lo plane needs the uniform-step GEMM form");
    // fewer than three MFMAs per product on the uniform-step loader only, and never with the activations alone as plain
    // f16: the call then runs at full precision (never less accurate than asked)
    const bool reduced = a.fastk && !a.cswap && (a.nm == 1 || a.nm == 2 || a.nm == 5);
    *plan = dma_plan(2, 2, 2, 2, true, a.fastk, a.cswap, reduced ? a.nm : 3, false, a.out_h16);
    plan->add_rows = a.ksplit == 2;    // (two work items per tile, one per half of K: the halves are added afterwards)
    // The 64-channel-step instantiations hold a second walk of the tile space (gemm_resident_walk.h, "resident-A walk"):
    // taken by a 1x1 over ONE source whose 128-row tile can be staged whole and held in registers - the correlation
    // GEMMs.  Longer K (the MemFlow read-out), a split K axis, two sources and every other product keep the streaming walk.
    plan->resident = plan->nm == 5 && plan->fastk && !plan->cswap && a.pointwise && a.ksplit == 1 && a.c1 == 0 &&
                     a.Kp <= VFML_RESIDENT_KMAX;
    return 0;
  }

  // Per-tap tile shape as TM TN WM WN digits: by output width, above 64 channels by the cost model
  int cfg = a.cout > 32 ? 2122 : 1141;
  if (a.cout > 64) {
    const double c3222 = dma_cost(a, 192, 128, 6.0, 1.0), c2322 = dma_cost(a, 128, 192, 6.0, 1.0),
                 c2222 = dma_cost(a, 128, 128, 4.0, 0.93), c2122 = dma_cost(a, 128, 64, 2.0, 0.7);
    cfg = 3222;
    double best = c3222;
    if (c2322 < best) { best = c2322; cfg = 2322; }
    if (c2222 < best) { best = c2222; cfg = 2222; }
    if (c2122 < best) { best = c2122; cfg = 2122; }
    if (a.proj_out && cfg != 3222 && cfg != 2222) cfg = c3222 <= c2222 ? 3222 : 2222;    // (128-column tiles of four waves)
  }
  bool forced = false;
  if (forced_tile && a.cout > 32) {
    // (2241 / 2341 exist in the shared-stage kernel only; narrower outputs keep their per-tap shapes otherwise)
    if (a.cout > 64 || forced_tile == 2241 || forced_tile == 2341) { cfg = forced_tile; forced = true; }
    VFML_REQUIRE(!a.proj_out || cfg == 3222 || cfg == 2222, "vfml_conv2d_split: proj_out runs on the 192 x 128 / 128 x 128 tiles (VFML_DMA_TILE)");
  }

  // stride-1 "same" convolutions with a filter row of 2..5 taps: one activation stage per (channel block, tap row),
  // shared by the row's taps (conv_gemm_tapx.hip).  The three-MFMA calls on the 192 x 128 / 128 x 192 tiles keep the
  // per-tap stages of conv_gemm_dma_kernel: there the two kernels run level.
  if (!(flags & VFML_CONV_PER_TAP) && !a.proj_out) {
    const int t = tapx_cfg(a, cfg, forced);
    if (t && (forced || a.nm == 5 || t == 2241 || t == 2341)) {
      *plan = tapx_plan(t / 1000, t / 100 % 10, t / 10 % 10, t % 10, a.nm);
      return 0;
    }
  }

  // The per-tap kernel on 16x16x32 MFMAs (MF16; measured against the 32x32x16 shape for the full-precision uniform-step
  // variants: 9-12 % faster on the 1080p update-block shapes - the chip holds a higher clock on it).
  // (a forced shared-stage shape on a call that kernel does not take runs 128 x 64; any other shape that is not built,
  // 128 x 128)
  if (cfg == 2241 || cfg == 2341) cfg = 2122;
  if (cfg != 3222 && cfg != 2322 && cfg != 2122 && cfg != 1141) cfg = 2222;
  // (the 128 x 32 tile has no uniform-step instantiation: such a call runs on the general loader, and so does every call
  // that does not qualify for uniform steps)
  const bool fastk = a.fastk && cfg != 1141;
  // (cannot happen: the validation picks 64-channel steps only where a uniform-step variant exists)
  VFML_REQUIRE(fastk || a.nm != 5, "vfml_conv2d_split: no 64-channel-step variant for this tile shape");
  *plan = dma_plan(cfg / 1000, cfg / 100 % 10, cfg / 10 % 10, cfg % 10, false, fastk, false, a.nm, true, false);
  return 0;
}

const SplitVariant* find_variant(const SplitVariant* rows, size_t n, const SplitPlan& p) {
  for (size_t i = 0; i < n; ++i) {
    const SplitPlan& k = rows[i].key;
    if (k.family == p.family && k.bn == p.bn && k.tm == p.tm && k.tn == p.tn && k.wm == p.wm && k.wn == p.wn && k.bigc == p.bigc &&
        k.in16 == p.in16 && k.persist == p.persist && k.fastk == p.fastk && k.cswap == p.cswap && k.mf16 == p.mf16 &&
        k.h16 == p.h16 && k.nm == p.nm)
      return &rows[i];
  }
  return nullptr;
}

int variant_name(const SplitPlan& k, char* buf, int len) {
  auto b = [](bool v) { return v ? "true" : "false"; };
  switch (k.family) {
    case SPLIT_REG:
      return snprintf(buf, len, "conv_gemm_split_kernel<%d, %d, %d, %s, %s, %d>", k.bn, k.wm, k.wn, b(k.bigc), b(k.in16), k.nm);
    case SPLIT_DMA:
      return snprintf(buf, len, "conv_gemm_dma_kernel<%d, %d, %d, %d, %s, %s, %s, %d, %s, %s>", k.tm, k.tn, k.wm, k.wn, b(k.persist),
                      b(k.fastk), b(k.cswap), k.nm, b(k.mf16), b(k.h16));
    default:
      return snprintf(buf, len, "conv_gemm_tapx_kernel<%d, %d, %d, %d, %d>", k.tm, k.tn, k.wm, k.wn, k.nm);
  }
}

}  // namespace vfml_detail
