// colour_defer_selftest -- csrc/pcp_colour_defer.hpp compiled for the host: the condition under which the whole-run colour call
// takes k_colour_pass_deferred (a 32-bit texel index spans the keyframe range).  CPU only.
// usage: colour_defer_selftest                      the built-in sweep; exit code 0 iff nothing disagrees
//        colour_defer_selftest B E PX [B E PX ...]  prints "fits B E PX: 0|1" for every triple (the test suite's edges)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../csrc/pcp_colour_defer.hpp"

// what the condition stands for: the largest index of the range, (E - B - 1) * PX + PX - 1, is a uint32, and the index the kernel
// forms in 32-bit arithmetic for keyframe f and pixel p is the 64-bit one
static bool largest_index_is_32_bit(int64_t b, int64_t e, int64_t px) {
  const unsigned __int128 last = static_cast<unsigned __int128>(e - b - 1) * static_cast<unsigned __int128>(px) + static_cast<unsigned __int128>(px - 1);
  return last <= 0xffffffffu;
}

int main(int argc, char **argv) {
  if (argc > 1) {
    if ((argc - 1) % 3 != 0) {
      std::fprintf(stderr, "usage: colour_defer_selftest [B E PX ...]\n");
      return 2;
    }
    for (int a = 1; a + 2 < argc; a += 3) {
      const long long b = std::atoll(argv[a]), e = std::atoll(argv[a + 1]), px = std::atoll(argv[a + 2]);
      std::printf("fits %lld %lld %lld: %d\n", b, e, px, pcp::deferred_index_fits(static_cast<int32_t>(b), static_cast<int32_t>(e), px) ? 1 : 0);
    }
    return 0;
  }
  long long cases = 0, mismatches = 0;
  const int64_t sizes[] = {3, 64 * 36, 640 * 360, 1920 * 1080, 4096 * 3000, 65536, 65537, (INT64_C(1) << 31) - 1};
  for (const int64_t px : sizes) {
    const int64_t edge = (INT64_C(1) << 32) / px;  // the longest range that fits
    for (int64_t len = edge > 3 ? edge - 3 : 1; len <= edge + 3 && len < (INT64_C(1) << 31) - 8; ++len) {
      for (const int64_t b : {INT64_C(0), INT64_C(1), INT64_C(7)}) {
        const bool got = pcp::deferred_index_fits(static_cast<int32_t>(b), static_cast<int32_t>(b + len), px);
        const bool want = largest_index_is_32_bit(b, b + len, px);
        cases += 1;
        if (got != want) {
          mismatches += 1;
          std::printf("MISMATCH [%lld, %lld) x %lld: %d, want %d\n", static_cast<long long>(b), static_cast<long long>(b + len),
                      static_cast<long long>(px), got, want);
        }
        // the 32-bit arithmetic of the kernel at the range's last texel
        if (got) {
          const uint32_t idx = static_cast<uint32_t>(len - 1) * static_cast<uint32_t>(px) + static_cast<uint32_t>(px - 1);
          if (static_cast<int64_t>(idx) != (len - 1) * px + px - 1) {
            mismatches += 1;
            std::printf("MISMATCH index [%lld, %lld) x %lld\n", static_cast<long long>(b), static_cast<long long>(b + len), static_cast<long long>(px));
          }
        }
      }
    }
  }
  // ranges and sizes that are no range or no image never fit
  const bool none = pcp::deferred_index_fits(5, 5, 100) || pcp::deferred_index_fits(6, 5, 100) || pcp::deferred_index_fits(-1, 5, 100) ||
                    pcp::deferred_index_fits(0, 5, 0) || pcp::deferred_index_fits(0, 5, -4) || pcp::deferred_index_fits(0, 1, INT64_C(1) << 31);
  cases += 6;
  if (none) {
    mismatches += 1;
    std::printf("MISMATCH: an empty or negative range, or an image of no or too many pixels, fits\n");
  }
  std::printf("colour_defer_selftest: %lld cases, %lld mismatches\n", cases, mismatches);
  return mismatches == 0 ? 0 : 1;
}
