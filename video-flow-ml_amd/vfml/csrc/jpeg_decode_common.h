// What the two JPEG decoders (jpeg_decode.hip: a wave per restart interval; jpeg_decode_sync.hip: a lane per subsequence
// of the scan) share: the argument block of their kernels, the workspace regions they have in common, the window of MCU
// rows a row range needs, and the launches of the marker kernels (count, place) and of the picture kernels (transform,
// colour), which live in jpeg_decode.hip.
#pragma once
#include "vfml_common.h"

namespace vfml_jpeg {

constexpr int kChunk = 4096;              // bytes of the scan per workgroup of the marker kernels
constexpr int kChunkThreads = 256;        // 16 bytes each
constexpr int kTableInts = 8 + 4 * 96;

enum { kErrCount = 1, kErrSequence = 2, kErrCode = 4, kErrIndex = 8, kErrData = 16 };

// The sampling (include/vfml.h VFML_JPEG_*).  An MCU holds `ny` luma blocks, hs across and vs down, then - but for grey -
// one block of Cb and one of Cr: nb blocks of 64 coefficients, in the order of the stream.
enum { kS420 = 0, kS422 = 1, kS444 = 2, kSGrey = 3 };
__host__ __device__ constexpr bool samp_ok(int s) { return s >= kS420 && s <= kSGrey; }
__host__ __device__ constexpr int samp_hs(int s) { return s == kS420 || s == kS422 ? 2 : 1; }
__host__ __device__ constexpr int samp_vs(int s) { return s == kS420 ? 2 : 1; }
__host__ __device__ constexpr int samp_ny(int s) { return samp_hs(s) * samp_vs(s); }
__host__ __device__ constexpr int samp_nb(int s) { return s == kSGrey ? 1 : samp_ny(s) + 2; }

struct DecArgs {
  const unsigned char* scan;
  unsigned n;                             // bytes of the scan
  int h, w, rows, cols;                   // picture; MCU rows, MCUs per row
  int samp, nb, ny;                       // sampling; blocks per MCU, luma blocks among them
  int ri, nint;                           // MCUs per interval (the whole picture when the file's Ri is 0), intervals
  const unsigned char* qt;                // [3][64] natural order
  const int* tables;                      // [kTableInts]
  int y0, y1;                             // output rows
  int int0;                               // first interval that is decoded
  int mrow0, mrows;                       // MCU rows that are transformed
  unsigned* bcount;                       // [chunks] markers per chunk
  unsigned* mpos;                         // [nint - 1] offset of the marker behind interval i
  short* coef;                            // [MCUs][nb][64] natural order
  unsigned char *py, *pcb, *pcr;          // planes [rows 8 vs][cols 8 hs], [rows 8][cols 8] x 2 (grey: luma alone)
  unsigned char* rgb;                     // row y0
  int64_t stride;
  int* status;
};

__host__ __device__ inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

struct DecLayout {
  int rows, cols;
  int64_t chunks, bcount, mpos, coef, py, pcb, pcr, bytes;
};

inline bool dec_layout(int h, int w, int samp, int64_t scan_bytes, DecLayout& L) {
  if (h < 1 || w < 1 || h > 65535 || w > 65535 || scan_bytes < 0 || scan_bytes > 0x7FFFFFFFll || !samp_ok(samp)) return false;
  const int mh = 8 * samp_vs(samp), mw = 8 * samp_hs(samp);
  L.rows = (h + mh - 1) / mh, L.cols = (w + mw - 1) / mw;
  const int64_t nmcu = (int64_t)L.rows * L.cols;
  L.chunks = scan_bytes > 0 ? (scan_bytes + kChunk - 1) / kChunk : 1;
  int64_t at = 0;
  L.bcount = at, at += align256(L.chunks * 4);
  L.mpos = at, at += align256(nmcu * 4);                        // Ri = 1: a marker per MCU
  L.coef = at, at += align256(nmcu * samp_nb(samp) * 64 * 2);
  L.py = at, at += align256(nmcu * samp_ny(samp) * 64);
  const int64_t chroma = samp == kSGrey ? 0 : nmcu * 64;
  L.pcb = at, at += align256(chroma);
  L.pcr = at, at += align256(chroma);
  L.bytes = at;
  return true;
}


// the MCU rows that rows y0 <= y < y1 need: their luma rows and, in 4:2:0, the chroma rows the triangle filter reads
// (the other samplings filter along a row or not at all)
inline void dec_window(DecArgs& a, int h, int y0, int y1) {
  if (a.samp != kS420) {
    a.mrow0 = y0 / 8, a.mrows = (y1 - 1) / 8 - a.mrow0 + 1;
    return;
  }
  const int ch = (h + 1) / 2;
  const int c0 = (y0 >> 1) - 1 > 0 ? (y0 >> 1) - 1 : 0;
  const int c1 = ((y1 - 1) >> 1) + 1 < ch - 1 ? ((y1 - 1) >> 1) + 1 : ch - 1;
  const int mlo = y0 / 16 < c0 / 8 ? y0 / 16 : c0 / 8;
  const int mhi = (y1 - 1) / 16 > c1 / 8 ? (y1 - 1) / 16 : c1 / 8;
  a.mrow0 = mlo, a.mrows = mhi - mlo + 1;
}

// what both entry points fill alike; the workspace regions follow L
inline void dec_args(DecArgs& a, const DecLayout& L, unsigned char* ws, const unsigned char* scan, int64_t scan_bytes, int h,
                     int w, int samp, int restart_interval, const unsigned char* qtables, const int32_t* tables, int y0,
                     int y1, unsigned char* rgb, int64_t row_stride, int32_t* status) {
  const int nmcu = L.rows * L.cols;
  a.scan = scan, a.n = (unsigned)scan_bytes, a.h = h, a.w = w, a.rows = L.rows, a.cols = L.cols;
  a.samp = samp, a.nb = samp_nb(samp), a.ny = samp_ny(samp);
  a.ri = restart_interval > 0 ? restart_interval : nmcu;
  a.nint = (nmcu + a.ri - 1) / a.ri;
  a.qt = qtables, a.tables = tables, a.y0 = y0, a.y1 = y1;
  a.bcount = reinterpret_cast<unsigned*>(ws + L.bcount);
  a.mpos = reinterpret_cast<unsigned*>(ws + L.mpos);
  a.coef = reinterpret_cast<short*>(ws + L.coef);
  a.py = ws + L.py, a.pcb = ws + L.pcb, a.pcr = ws + L.pcr;
  a.rgb = rgb, a.stride = row_stride, a.status = status;
  a.int0 = 0;
  dec_window(a, h, y0, y1);
}

// jpeg_decode.hip: count + place (status, bcount, mpos), transform + colour (coef -> planes -> rgb), on stream s
__attribute__((visibility("hidden"))) void dec_launch_markers(const DecArgs& a, unsigned chunks, hipStream_t s);
__attribute__((visibility("hidden"))) void dec_launch_picture(const DecArgs& a, hipStream_t s);

}  // namespace vfml_jpeg
