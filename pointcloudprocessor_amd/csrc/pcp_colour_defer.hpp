// pcp_colour_defer.hpp -- the host's condition for k_colour_pass_deferred (pcp_colour.hip), plain C++ so that
// host/colour_defer_selftest.cpp checks the same text the library compiles.
#pragma once

#include <stdint.h>

namespace pcp {

// The deferred list names a texel by the 32-bit index (f - frame_begin) * image_px + pixel, pixel < image_px: the largest one is
// (frame_end - frame_begin) * image_px - 1, which fits while the product is at most 2^32 -- 2071 keyframes at 1920 x 1080, 349
// at 4096 x 3000.  (Both factors are below 2^31: the product cannot overflow an int64.)
inline bool deferred_index_fits(int32_t frame_begin, int32_t frame_end, int64_t image_px) {
  if (frame_begin < 0 || frame_end <= frame_begin || image_px <= 0 || image_px > INT64_C(0x7fffffff)) return false;
  return static_cast<int64_t>(frame_end - frame_begin) * image_px <= (INT64_C(1) << 32);
}

}  // namespace pcp
