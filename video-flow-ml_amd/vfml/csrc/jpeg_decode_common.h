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

struct DecArgs {
  const unsigned char* scan;
  unsigned n;                             // bytes of the scan
  int h, w, rows, cols;                   // picture; MCU rows, MCUs per row
  int ri, nint;                           // MCUs per interval (the whole picture when the file's Ri is 0), intervals
  const unsigned char* qt;                // [3][64] natural order
  const int* tables;                      // [kTableInts]
  int y0, y1;                             // output rows
  int int0;                               // first interval that is decoded
  int mrow0, mrows;                       // MCU rows that are transformed
  unsigned* bcount;                       // [chunks] markers per chunk
  unsigned* mpos;                         // [nint - 1] offset of the marker behind interval i
  short* coef;                            // [MCUs][6][64] natural order
  unsigned char *py, *pcb, *pcr;          // planes [16 rows][16 cols], [8 rows][8 cols] x 2
  unsigned char* rgb;                     // row y0
  int64_t stride;
  int* status;
};

__host__ __device__ inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

struct DecLayout {
  int rows, cols;
  int64_t chunks, bcount, mpos, coef, py, pcb, pcr, bytes;
};

inline bool dec_layout(int h, int w, int64_t scan_bytes, DecLayout& L) {
  if (h < 1 || w < 1 || h > 65535 || w > 65535 || scan_bytes < 0 || scan_bytes > 0x7FFFFFFFll) return false;
  L.rows = (h + 15) / 16, L.cols = (w + 15) / 16;
  const int64_t nmcu = (int64_t)L.rows * L.cols;
  L.chunks = scan_bytes > 0 ? (scan_bytes + kChunk - 1) / kChunk : 1;
  int64_t at = 0;
  L.bcount = at, at += align256(L.chunks * 4);
  L.mpos = at, at += align256(nmcu * 4);                        // Ri = 1: a marker per MCU
  L.coef = at, at += align256(nmcu * 6 * 64 * 2);
  L.py = at, at += align256(nmcu * 256);
  L.pcb = at, at += align256(nmcu * 64);
  L.pcr = at, at += align256(nmcu * 64);
  L.bytes = at;
  return true;
}


// the MCU rows that rows y0 <= y < y1 need: their luma rows and the chroma rows the triangle filter reads
inline void dec_window(DecArgs& a, int h, int y0, int y1) {
  const int ch = (h + 1) / 2;
  const int c0 = (y0 >> 1) - 1 > 0 ? (y0 >> 1) - 1 : 0;
  const int c1 = ((y1 - 1) >> 1) + 1 < ch - 1 ? ((y1 - 1) >> 1) + 1 : ch - 1;
  const int mlo = y0 / 16 < c0 / 8 ? y0 / 16 : c0 / 8;
  const int mhi = (y1 - 1) / 16 > c1 / 8 ? (y1 - 1) / 16 : c1 / 8;
  a.mrow0 = mlo, a.mrows = mhi - mlo + 1;
}

// jpeg_decode.hip: count + place (status, bcount, mpos), transform + colour (coef -> planes -> rgb), on stream s
__attribute__((visibility("hidden"))) void dec_launch_markers(const DecArgs& a, unsigned chunks, hipStream_t s);
__attribute__((visibility("hidden"))) void dec_launch_picture(const DecArgs& a, hipStream_t s);

}  // namespace vfml_jpeg
