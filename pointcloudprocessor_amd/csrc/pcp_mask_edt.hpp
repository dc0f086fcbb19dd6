// pcp_mask_edt.hpp -- the per-element arithmetic of the mask distance maps ("Mask distance maps", MD1-MD6), one
// copy for the kernels (pcp_mask_edt.hip) and the CPU form (pcp_mask_edt_host).  Everything is integer: the squared
// distance is exact, and the winner among equally distant background pixels is the one with the lowest linear index.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCP_MD_HD __host__ __device__ __forceinline__
#else
#define PCP_MD_HD inline
#endif

namespace pcp {
namespace md {

constexpr int32_t kMaxSide = 16384;           // MD6: W, H <= 2^14, so dx^2, dy^2 < 2^28 and d2 < 2^29
constexpr int32_t kSegmentRows = 64;          // column stage: rows per segment (one 64-bit background mask per column)
constexpr uint32_t kNoColumn = 0x8000ffffu;   // column word of a column without a background pixel: dy = 2^15, row 0xffff
constexpr uint32_t kNoneD2 = 0x40000000u;     // = (2^15)^2: a candidate of such a column is at least this far (saturates, never wraps)
constexpr uint32_t kSentinelD2 = 0xffffffffu; // MD5: results of a mask without a background pixel
constexpr int32_t kSentinelNearest = -1;

// MD1: foreground iff the mask byte exceeds the threshold (cv2.threshold(mask, t, 255, THRESH_BINARY))
PCP_MD_HD bool foreground(uint32_t mask_byte, int32_t threshold) { return static_cast<int32_t>(mask_byte) > threshold; }

// MD3, column stage.  `up` = row of the nearest background pixel at or above row y of the column, `down` = at or below it
// (-1: none).  Ties go to the UPPER row: of two pixels of one column at the same distance the upper has the lower index.
PCP_MD_HD int32_t column_pick(int32_t y, int32_t up, int32_t down) {
  if (up < 0) return down;
  if (down < 0) return up;
  return (y - up) <= (down - y) ? up : down;
}

// the column word of pixel (x, y): vertical distance << 16 | row of that background pixel; kNoColumn for row < 0
PCP_MD_HD uint32_t column_word(int32_t y, int32_t row) {
  if (row < 0) return kNoColumn;
  const int32_t dy = row > y ? row - y : y - row;
  return (static_cast<uint32_t>(dy) << 16) | static_cast<uint32_t>(row);
}

// MD2 + MD4, row stage: the 64-bit key of the candidate "nearest background pixel of column xc" seen from a pixel dx
// columns away: (dx^2 + dy^2) << 32 | row * W + xc.  The smallest key over all columns is the result.  A column without
// background gives a key of at least kNoneD2 << 32, above every real one.
PCP_MD_HD unsigned long long candidate_key(uint32_t word, int32_t dx, int32_t xc, int32_t width) {
  const uint32_t dy = word >> 16, row = word & 0xffffu;
  const uint32_t d2 = static_cast<uint32_t>(dx * dx) + dy * dy;
  const uint32_t index = row * static_cast<uint32_t>(width) + static_cast<uint32_t>(xc);
  return (static_cast<unsigned long long>(d2) << 32) | index;
}

// The row stage of one pixel: candidates outward from its own column, both sides per step, until dx^2 EXCEEDS the best
// d2 (a candidate at dx^2 == best d2 may still win on the index).  At most `width` steps for any mask.
template <typename Row>
PCP_MD_HD unsigned long long row_search(const Row &row, int32_t x, int32_t width) {
  unsigned long long best = candidate_key(row[x], 0, x, width);
  for (int32_t r = 1; r < width; ++r) {
    if (static_cast<uint32_t>(r * r) > static_cast<uint32_t>(best >> 32)) break;
    const int32_t xl = x - r, xr = x + r;
    if (xl < 0 && xr >= width) break;
    if (xl >= 0) {
      const unsigned long long k = candidate_key(row[xl], r, xl, width);
      best = k < best ? k : best;
    }
    if (xr < width) {
      const unsigned long long k = candidate_key(row[xr], r, xr, width);
      best = k < best ? k : best;
    }
  }
  return best;
}

// MD5: the outputs of a key
PCP_MD_HD uint32_t key_d2(unsigned long long key) {
  const uint32_t d2 = static_cast<uint32_t>(key >> 32);
  return d2 >= kNoneD2 ? kSentinelD2 : d2;
}
PCP_MD_HD int32_t key_nearest(unsigned long long key) {
  return static_cast<uint32_t>(key >> 32) >= kNoneD2 ? kSentinelNearest : static_cast<int32_t>(static_cast<uint32_t>(key));
}

}  // namespace md
}  // namespace pcp
