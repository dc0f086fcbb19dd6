// pcp_ortho_defects.hpp -- the per-pixel arithmetic of the surface defects on ortho maps ("Surface defects on ortho
// maps", SD1-SD9), one copy for the kernels (pcp_ortho_defects.hip), the CPU form (pcp_ortho_defects_host) and
// host/ortho_defects_selftest.cpp.  Integers throughout: a depth becomes a quantum of 2^-20 m, the window sums are prefix
// sums modulo 2^64 (exact: the true sums stay below 2^52), and every comparison is made without a division.
#pragma once

#include <cmath>
#include <cstdint>

#include "pcp_ortho.hpp"

namespace pcp {
namespace sd {

constexpr int kQuantumBits = 20;                 // SD2: a quantum is 2^-20 m
constexpr double kQuanta = 1048576.0;            // 2^20
constexpr float kMaxDepth = 512.0f;              // SD2
constexpr float kMinThreshold = 0x1p-20f, kMaxThreshold = 1.0f;  // SD1
constexpr int32_t kMaxWindow = 1024;             // SD1
constexpr int kRowWords = 16;                    // SD7
constexpr int kOutWords = 8;                     // SD8
// SD7: the columns of a region's row
enum { R_CLASS = 0, R_PIXELS, R_MEASURED, R_SUM, R_MAX, R_MAX_PIXEL, R_COL_MIN, R_COL_MAX, R_ROW_MIN, R_ROW_MAX, R_SUM_COL, R_SUM_ROW,
       R_OPEN, R_FIRST, R_FIRST_PASS, R_ZERO };
// SD8: the counts of a call
enum { O_KEPT = 0, O_DROPPED, O_HOLLOW, O_BULGE, O_UNSUPPORTED, O_REFUSED, O_FIRST_PASS, O_SURFACE };
// the flags of a pixel
constexpr uint8_t kSurface = 1, kMeasured = 2, kFirstPass = 4;

// SD1 after the checks: T in quanta, the rest as the caller gave it
struct Params {
  int64_t T;
  int32_t W, refine, min_support, min_pixels, classes;
};

// SD1: nullptr, or the name of the first field that is out of range
inline const char *bad_field(float threshold, int32_t window_px, int32_t refine, int32_t min_support, int32_t min_pixels, int32_t classes) {
  if (!(om::finite_bits(threshold) && threshold >= kMinThreshold && threshold <= kMaxThreshold)) return "threshold";
  if (window_px < 0 || window_px > kMaxWindow) return "window_px";
  if (refine != 0 && refine != 1) return "refine";
  if (refine == 1 && window_px == 0) return "refine";
  if (window_px > 0 && min_support < 1) return "min_support";
  if (min_pixels < 1) return "min_pixels";
  if (classes < 1 || classes > 3) return "classes";
  return nullptr;
}

// SD2: exact scaling, ties to even
PCP_OM_HD int64_t quanta_of(float metres) { return static_cast<int64_t>(llrint(static_cast<double>(metres) * kQuanta)); }

// SD2: whether a pixel of this status and depth is surface, and its quantum; *refused: it has a status but its depth is not taken
PCP_OM_HD bool surface(uint32_t status, float depth, int32_t *q, bool *refused) {
  *q = 0;
  *refused = false;
  if (status != 1u && status != 2u) return false;
  if (!(om::finite_bits(depth) && depth >= -kMaxDepth && depth <= kMaxDepth)) {
    *refused = true;
    return false;
  }
  *q = static_cast<int32_t>(quanta_of(depth));
  return true;
}

// SD3: the sum over rows r0..r1 and columns c0..c1 (inside the raster) of an inclusive summed-area table, modulo 2^64
PCP_OM_HD uint64_t box_sum(const unsigned long long *sat, int32_t w, int32_t r0, int32_t r1, int32_t c0, int32_t c1) {
  const int64_t w64 = w;
  uint64_t s = sat[r1 * w64 + c1];
  if (r0 > 0) s -= sat[(r0 - 1) * w64 + c1];
  if (c0 > 0) s -= sat[r1 * w64 + (c0 - 1)];
  if (r0 > 0 && c0 > 0) s += sat[(r0 - 1) * w64 + (c0 - 1)];
  return s;
}

// SD3: S and n of pixel (r, c)'s window, clipped to the raster; sat_q and sat_n are the two tables
PCP_OM_HD void window(const unsigned long long *sat_q, const unsigned long long *sat_n, int32_t w, int32_t h, int32_t r, int32_t c, int32_t W,
                      int64_t *S, int64_t *n) {
  const int32_t r0 = r - W < 0 ? 0 : r - W, r1 = r + W > h - 1 ? h - 1 : r + W;
  const int32_t c0 = c - W < 0 ? 0 : c - W, c1 = c + W > w - 1 ? w - 1 : c + W;
  *S = static_cast<int64_t>(box_sum(sat_q, w, r0, r1, c0, c1));
  *n = static_cast<int64_t>(box_sum(sat_n, w, r0, r1, c0, c1));
}

// SD3: the class (every class bit on) and the deviation of a supported pixel (n >= 1)
PCP_OM_HD int32_t classify(int64_t q, int64_t S, int64_t n, int64_t T, int32_t *dev) {
  const int64_t e = q * n - S;
  *dev = static_cast<int32_t>(e / n);  // (C's division truncates)
  return e >= T * n ? 1 : (e <= -(T * n) ? 2 : 0);
}

// SD3b
PCP_OM_HD int32_t classify_frame(int64_t q, int64_t T) { return q >= T ? 1 : (q <= -T ? 2 : 0); }

// the class after the mask (bit 0 hollows, bit 1 bulges)
PCP_OM_HD int32_t masked(int32_t cls, int32_t classes) { return (cls && ((classes >> (cls - 1)) & 1)) ? cls : 0; }

// SD6: the word whose maximum over a region gives the greatest |dev| and, among equals, the lowest pixel
PCP_OM_HD uint64_t best_word(int32_t dev, int64_t pixel) {
  const uint64_t a = static_cast<uint64_t>(dev < 0 ? -static_cast<int64_t>(dev) : static_cast<int64_t>(dev));
  return (a << 32) | (0xffffffffull - static_cast<uint64_t>(pixel));
}
PCP_OM_HD int64_t best_abs(uint64_t word) { return static_cast<int64_t>(word >> 32); }
PCP_OM_HD int64_t best_pixel(uint64_t word) { return static_cast<int64_t>(0xffffffffull - (word & 0xffffffffull)); }

// SD7: whether pixel (r, c) is open: on the raster's edge, or a 4-neighbour is no surface pixel
PCP_OM_HD bool open_pixel(const uint8_t *flags, int32_t w, int32_t h, int32_t r, int32_t c) {
  if (r == 0 || c == 0 || r == h - 1 || c == w - 1) return true;
  const int64_t p = static_cast<int64_t>(r) * w + c;
  return !((flags[p - 1] & flags[p + 1] & flags[p - w] & flags[p + w]) & kSurface);
}

}  // namespace sd
}  // namespace pcp
