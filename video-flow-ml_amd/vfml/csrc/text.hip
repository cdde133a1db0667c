// Text labels of the output video ("Text"): vfml_text_draw draws a compiled draw list - strings of
// the project's stroke font and dimmed rectangles - into a composed u8 frame in place, between vfml_compose_frame and the
// JPEG encoder or the copy back.  Integer only; byte for byte tests/text_oracle.py and visualization/text.py.
//
// Blending is ordered and reads the destination, and a label's outline and fill (a legend number's shadow and text, two
// neighbouring labels) overlap.  So the plan carries disjoint pixel BOXES, each with its operations in draw order; one
// thread owns one pixel of one box, walks the box's operations in order with the pixel in registers and stores it once.
// No pixel is touched by two threads; there are no atomics and no second pass.
//
// A block belongs to one box, so everything read from the plan - operations, glyph boxes, segments - is uniform across
// the block and comes through the scalar cache; nothing is staged in LDS.  A block covers 32 x 8 pixels of its box, each
// of its four waves an 8 x 8 tile: a tile meets one or two glyphs of a label, and a wave whose lanes all fail a cull
// skips the work behind it.  Per operation a thread culls each glyph by its bounding box (grown by the stroke radius),
// then each segment by its own, before it tests the segment, 16 samples per pixel when anti-aliased.  Segments are read
// four at a time (the last one repeated past the end, which changes nothing): one load latency per four, not per one.
//
// The entry point checks the plan's host words completely before the launch (vfml.h).  The kernel reads the device copy
// and still bounds every count, offset and coordinate it takes from it against plan_words and the image: whatever those
// words hold, no access leaves the plan or the image.
#include "vfml_common.h"

namespace {

constexpr int kMagic = 0x54584656;                        // "VFXT"
constexpr int kHeader = 8, kBoxWords = 8, kOpWords = 12, kGlyphWords = 8, kSegWords = 4;
constexpr int kBlock = 256, kBlockW = 32, kBlockH = 8;    // a block's pixels: four 8 x 8 wave tiles side by side
constexpr int kMaxBoxes = 4096, kMaxOps = 65536, kMaxGlyphs = 1 << 20, kMaxSegs = 1 << 22;
constexpr int kMaxRadius = 512;                           // thickness 16
constexpr int kMaxRel = 1 << 24;                          // |string-relative coordinate|, 1/64 px
constexpr int kMaxExtent = 1 << 14;                       // a glyph's width and height, 1/64 px (font_scale <= 8)
constexpr int kMaxOrigin = 1 << 26;
constexpr int kMaxBlocks = 1 << 20;

struct TextArgs {
  const int* plan;        // device copy
  int words;
  unsigned char* img;
  int h, w;
  int64_t stride;
  int bottom_up;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sample q = p - a against segment d = b - a: within r of it.  |q| < 2^15 and |d| <= 2^14 behind the glyph cull, so u, c
// and L2 are below 2^31; only c^2 and r^2 L2 need 64 bits.
__device__ __forceinline__ bool sample_inside(int qx, int qy, int dx, int dy, int L2, int r2, int64_t r2L2) {
  const int u = qx * dx + qy * dy;
  if (u <= 0) return qx * qx + qy * qy <= r2;
  if (u >= L2) {
    const int ex = qx - dx, ey = qy - dy;
    return ex * ex + ey * ey <= r2;
  }
  const int c = qx * dy - qy * dx;
  return (int64_t)c * c <= r2L2;
}

__global__ __launch_bounds__(kBlock) void text_draw_kernel(const TextArgs a) {
  const int* __restrict__ P = a.plan;
  if (a.words < kHeader) return;
  const int nb = P[4], no = P[5], ng = P[6], ns = P[7];
  if (nb < 0 || nb > kMaxBoxes || no < 0 || no > kMaxOps || ng < 0 || ng > kMaxGlyphs || ns < 0 || ns > kMaxSegs) return;
  const int boxes = kHeader, ops = boxes + kBoxWords * nb, glyphs = ops + kOpWords * no;
  const int64_t segs64 = (int64_t)glyphs + (int64_t)kGlyphWords * ng;
  if (segs64 + (int64_t)kSegWords * ns > (int64_t)a.words) return;
  const int segs = (int)segs64;

  // this block's box
  const int blk = (int)blockIdx.x;
  int x0 = 0, y0 = 0, x1 = 0, y1 = 0, bcols = 1, op_first = 0, op_count = 0;
  int64_t base = 0;
  bool found = false;
  for (int k = 0; k < nb && !found; ++k) {
    const int* B = P + boxes + kBoxWords * k;
    const int bx0 = clampi(B[0], 0, a.w - 1), by0 = clampi(B[1], 0, a.h - 1);
    const int bx1 = clampi(B[2], 0, a.w - 1), by1 = clampi(B[3], 0, a.h - 1);
    if (bx1 < bx0 || by1 < by0) continue;
    const int cols = (bx1 - bx0 + kBlockW) / kBlockW, rows = (by1 - by0 + kBlockH) / kBlockH;
    const int64_t first = B[6], nblk = (int64_t)cols * rows;
    if (blk >= first && blk < first + nblk) {
      found = true;
      x0 = bx0; y0 = by0; x1 = bx1; y1 = by1; bcols = cols;
      base = blk - first;
      op_first = clampi(B[4], 0, no);
      op_count = clampi(B[5], 0, no - op_first);
    }
  }
  if (!found) return;
  const int tid = (int)threadIdx.x;
  const int px = x0 + (int)(base % bcols) * kBlockW + (tid >> 6) * 8 + (tid & 7);
  const int py = y0 + (int)(base / bcols) * kBlockH + ((tid >> 3) & 7);
  if (px > x1 || py > y1) return;
  const int row = a.bottom_up ? a.h - 1 - py : py;
  unsigned char* pix = a.img + (int64_t)row * a.stride + 3 * (int64_t)px;
  int c0 = pix[0], c1 = pix[1], c2 = pix[2];
  bool touched = false;

  for (int o = op_first; o < op_first + op_count; ++o) {
    const int* O = P + ops + kOpWords * o;
    if (px < O[1] || py < O[2] || px > O[3] || py > O[4]) continue;          // the operation's clip
    if (O[0] == 1) {                                                          // DIM_RECT
      c0 = (3 * c0 + 5) / 10; c1 = (3 * c1 + 5) / 10; c2 = (3 * c2 + 5) / 10;
      touched = true;
      continue;
    }
    if (O[0] != 0) continue;
    const unsigned colour = (unsigned)O[5];
    const int r = clampi(O[6], 0, kMaxRadius), aa = O[7] != 0;
    const int r2 = r * r;
    // the pixel's corner relative to the string's origin, 1/64 px
    const int64_t ux64 = 64 * (int64_t)px - O[8], uy64 = 64 * (int64_t)py - O[9];
    const int g_first = clampi(O[10], 0, ng), g_count = clampi(O[11], 0, ng - g_first);
    unsigned mask = 0;                                                        // bit 4 j + i: sample (i, j) is inside
    for (int g = g_first; g < g_first + g_count; ++g) {
      const int* G = P + glyphs + kGlyphWords * g;
      const int gx0 = clampi(G[0], -kMaxRel, kMaxRel), gy0 = clampi(G[1], -kMaxRel, kMaxRel);
      const int gx1 = clampi(G[2], gx0, gx0 + kMaxExtent), gy1 = clampi(G[3], gy0, gy0 + kMaxExtent);
      if (ux64 + 63 < gx0 - r || ux64 > gx1 + r || uy64 + 63 < gy0 - r || uy64 > gy1 + r) continue;
      const int ux = (int)(ux64 - gx0), uy = (int)(uy64 - gy0);             // relative to the glyph's box from here on
      const int s_first = clampi(G[4], 0, ns), s_count = clampi(G[5], 0, ns - s_first);
      const int s_last = s_first + s_count - 1;
      for (int s4 = s_first; s4 <= s_last; s4 += 4) {
        int sa[4][4];                                                         // four segments' words, loaded together
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int* S = P + segs + kSegWords * (s4 + j < s_last ? s4 + j : s_last);
          sa[j][0] = S[0]; sa[j][1] = S[1]; sa[j][2] = S[2]; sa[j][3] = S[3];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ax = clampi(sa[j][0], gx0, gx1) - gx0, ay = clampi(sa[j][1], gy0, gy1) - gy0;
          const int bx = clampi(sa[j][2], gx0, gx1) - gx0, by = clampi(sa[j][3], gy0, gy1) - gy0;
          // the pixel's units [u, u + 63] against the segment's box grown by r
          if (ux + 63 < (ax < bx ? ax : bx) - r || ux > (ax > bx ? ax : bx) + r || uy + 63 < (ay < by ? ay : by) - r ||
              uy > (ay > by ? ay : by) + r)
            continue;
          const int dx = bx - ax, dy = by - ay;
          const int L2 = dx * dx + dy * dy;
          const int64_t r2L2 = (int64_t)r2 * L2;
          if (aa) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
              const int qx = ux + 4 * (2 * (k & 3) + 1) - ax, qy = uy + 4 * (2 * (k >> 2) + 1) - ay;
              if (sample_inside(qx, qy, dx, dy, L2, r2, r2L2)) mask |= 1u << k;
            }
          } else if (sample_inside(ux + 32 - ax, uy + 32 - ay, dx, dy, L2, r2, r2L2)) {
            mask = 0xffffu;
          }
        }
      }
    }
    if (mask) {
      const int n = __popc(mask);
      c0 = ((int)(colour & 255u) * n + c0 * (16 - n) + 8) >> 4;
      c1 = ((int)((colour >> 8) & 255u) * n + c1 * (16 - n) + 8) >> 4;
      c2 = ((int)((colour >> 16) & 255u) * n + c2 * (16 - n) + 8) >> 4;
      touched = true;
    }
  }
  if (touched) {
    pix[0] = (unsigned char)c0;
    pix[1] = (unsigned char)c1;
    pix[2] = (unsigned char)c2;
  }
}

// 0, or 1 with the error set: the plan's host words are well-formed for an h x w image
int check_plan(const int32_t* P, int words, int h, int w) {
  VFML_REQUIRE(words >= kHeader, "vfml_text_draw: plan of %d words is shorter than its header", words);
  VFML_REQUIRE(P[0] == kMagic, "vfml_text_draw: plan does not start with the plan magic");
  const int nb = P[4], no = P[5], ng = P[6], ns = P[7];
  VFML_REQUIRE(nb >= 0 && nb <= kMaxBoxes && no >= 0 && no <= kMaxOps && ng >= 0 && ng <= kMaxGlyphs && ns >= 0 &&
                   ns <= kMaxSegs, "vfml_text_draw: plan counts %d / %d / %d / %d out of range", nb, no, ng, ns);
  const int64_t total = kHeader + (int64_t)kBoxWords * nb + (int64_t)kOpWords * no + (int64_t)kGlyphWords * ng +
                        (int64_t)kSegWords * ns;
  VFML_REQUIRE(total == (int64_t)words && P[1] == words,
               "vfml_text_draw: plan is truncated or padded: its sections need %lld words, its header says %d, %d given",
               (long long)total, P[1], words);
  const int32_t* B = P + kHeader;
  const int32_t* O = B + kBoxWords * nb;
  const int32_t* G = O + kOpWords * no;
  const int32_t* S = G + kGlyphWords * ng;
  int64_t blocks = 0;
  for (int k = 0; k < nb; ++k) {
    const int32_t* b = B + kBoxWords * k;
    VFML_REQUIRE(b[0] >= 0 && b[1] >= 0 && b[0] <= b[2] && b[1] <= b[3] && b[2] < w && b[3] < h,
                 "vfml_text_draw: box %d (%d, %d)..(%d, %d) outside the %d x %d image", k, b[0], b[1], b[2], b[3], w, h);
    VFML_REQUIRE(b[4] >= 0 && b[5] >= 1 && (int64_t)b[4] + b[5] <= no,
                 "vfml_text_draw: box %d has operations %d + %d of %d", k, b[4], b[5], no);
    VFML_REQUIRE(b[6] == blocks, "vfml_text_draw: box %d starts at block %d, not %lld", k, b[6], (long long)blocks);
    blocks += (int64_t)((b[2] - b[0] + kBlockW) / kBlockW) * ((b[3] - b[1] + kBlockH) / kBlockH);
    VFML_REQUIRE(blocks <= kMaxBlocks, "vfml_text_draw: boxes of more than %d blocks", kMaxBlocks);
    for (int j = 0; j < k; ++j) {
      const int32_t* c = B + kBoxWords * j;
      VFML_REQUIRE(b[0] > c[2] || c[0] > b[2] || b[1] > c[3] || c[1] > b[3],
                   "vfml_text_draw: boxes %d and %d intersect (one thread per pixel: boxes are disjoint)", j, k);
    }
  }
  for (int k = 0; k < no; ++k) {
    const int32_t* o = O + kOpWords * k;
    VFML_REQUIRE(o[0] == 0 || o[0] == 1, "vfml_text_draw: operation %d of unknown kind %d", k, o[0]);
    VFML_REQUIRE(o[1] >= 0 && o[2] >= 0 && o[1] <= o[3] && o[2] <= o[4] && o[3] < w && o[4] < h,
                 "vfml_text_draw: operation %d clip (%d, %d)..(%d, %d) outside the %d x %d image", k, o[1], o[2], o[3],
                 o[4], w, h);
    if (o[0] == 1) continue;
    VFML_REQUIRE((o[5] >> 24) == 0, "vfml_text_draw: operation %d colour 0x%x", k, o[5]);
    VFML_REQUIRE(o[6] >= 32 && o[6] <= kMaxRadius && o[6] % 32 == 0, "vfml_text_draw: operation %d radius %d", k, o[6]);
    VFML_REQUIRE(o[7] == 0 || o[7] == 1, "vfml_text_draw: operation %d anti-aliasing flag %d", k, o[7]);
    VFML_REQUIRE(o[8] >= -kMaxOrigin && o[8] <= kMaxOrigin && o[9] >= -kMaxOrigin && o[9] <= kMaxOrigin,
                 "vfml_text_draw: operation %d origin (%d, %d) out of range", k, o[8], o[9]);
    VFML_REQUIRE(o[10] >= 0 && o[11] >= 1 && (int64_t)o[10] + o[11] <= ng,
                 "vfml_text_draw: operation %d has glyphs %d + %d of %d", k, o[10], o[11], ng);
  }
  for (int k = 0; k < ng; ++k) {
    const int32_t* g = G + kGlyphWords * k;
    VFML_REQUIRE(g[0] >= -kMaxRel && g[1] >= -kMaxRel && g[0] <= g[2] && g[1] <= g[3] && g[2] <= kMaxRel &&
                     g[3] <= kMaxRel && g[2] - g[0] <= kMaxExtent && g[3] - g[1] <= kMaxExtent,
                 "vfml_text_draw: glyph %d box (%d, %d)..(%d, %d) out of range", k, g[0], g[1], g[2], g[3]);
    VFML_REQUIRE(g[4] >= 0 && g[5] >= 1 && (int64_t)g[4] + g[5] <= ns,
                 "vfml_text_draw: glyph %d has segments %d + %d of %d", k, g[4], g[5], ns);
    for (int j = g[4]; j < g[4] + g[5]; ++j) {
      const int32_t* s = S + kSegWords * j;
      VFML_REQUIRE(s[0] >= g[0] && s[0] <= g[2] && s[2] >= g[0] && s[2] <= g[2] && s[1] >= g[1] && s[1] <= g[3] &&
                       s[3] >= g[1] && s[3] <= g[3], "vfml_text_draw: segment %d leaves the box of glyph %d", j, k);
    }
  }
  return 0;
}

}  // namespace

extern "C" int vfml_text_draw(const int32_t* plan, int plan_words, unsigned char* img, int h, int w, int64_t row_stride,
                              int flags, void* stream) {
  VFML_REQUIRE(plan && img && h > 0 && w > 0 && h <= 65535 && w <= 65535, "vfml_text_draw: bad argument");
  VFML_REQUIRE((flags & ~VFML_COMPOSE_BOTTOM_UP) == 0, "vfml_text_draw: unknown flags 0x%x", flags);
  VFML_REQUIRE(row_stride >= 3 * (int64_t)w && row_stride < ((int64_t)1 << 31),
               "vfml_text_draw: row stride %lld below 3 * %d", (long long)row_stride, w);
  VFML_REQUIRE((reinterpret_cast<uintptr_t>(plan) & 3u) == 0, "vfml_text_draw: plan must be 4-byte aligned");
  if (check_plan(plan, plan_words, h, w) != 0) return 1;
  if (plan[4] == 0) return 0;                              // nothing to draw
  const uint64_t dev = (uint64_t)(uint32_t)plan[2] | ((uint64_t)(uint32_t)plan[3] << 32);
  VFML_REQUIRE(dev != 0 && (dev & 3u) == 0,
               "vfml_text_draw: plan words 2..3 do not hold the address of the plan's device copy");
  TextArgs a;
  a.plan = reinterpret_cast<const int*>(static_cast<uintptr_t>(dev));
  a.words = plan_words;
  a.img = img;
  a.h = h; a.w = w;
  a.stride = row_stride;
  a.bottom_up = (flags & VFML_COMPOSE_BOTTOM_UP) != 0;
  const int32_t* last = plan + kHeader + kBoxWords * (plan[4] - 1);
  const int64_t blocks = last[6] + (int64_t)((last[2] - last[0] + kBlockW) / kBlockW) * ((last[3] - last[1] + kBlockH) / kBlockH);
  hipLaunchKernelGGL(text_draw_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), a);
  return vfml_check_launch("vfml_text_draw");
}
