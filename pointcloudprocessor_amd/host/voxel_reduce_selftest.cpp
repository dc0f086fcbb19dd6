// voxel_reduce_selftest -- csrc/pcp_voxel_reduce.hpp compiled for the host (CPU only: never a GPU job).  Checks the cell / key
// round trip, floor division, the single-row identity (a voxel of one row with |x| >= 2^-9 returns the coordinate bit for
// bit; below, within 2^-33 m), and the centroid against the same quotient taken over the absolute fixed-point sums in
// 128-bit integers.  Prints the number of mismatches; exit code 0 iff none.   usage: voxel_reduce_selftest [count]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/pcp_voxel_reduce.hpp"

using namespace pcp;

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

static float unit(uint64_t r) { return static_cast<float>(static_cast<double>(r >> 11) * (1.0 / 9007199254740992.0)); }

int main(int argc, char **argv) {
  const uint64_t count = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 2000000ull;
  uint64_t bad = 0;
  auto fail = [&](const char *what, double a, double b) {
    if (bad < 10) std::fprintf(stderr, "mismatch (%s): %.17g %.17g\n", what, a, b);
    ++bad;
  };
  const float leaves[] = {1e-4f, 0.001f, 0.005f, 0.013f, 0.05f, 0.25f, 1.0f};
  // floor division on signed integers
  for (int64_t a = -40; a <= 40; ++a)
    for (int64_t b = 1; b <= 7; ++b)
      if (vg::floor_div(a, b) != static_cast<int64_t>(std::floor(static_cast<double>(a) / static_cast<double>(b)))) fail("floor_div", a, b);
  if (!vg::leaf_ok(1e-4f) || !vg::leaf_ok(1.0f) || vg::leaf_ok(9e-5f) || vg::leaf_ok(1.5f) || vg::leaf_ok(0.0f) || vg::leaf_ok(NAN))
    fail("leaf_ok", 0, 0);
  for (float leaf : leaves) {
    const float inv = vg::inverse_leaf(leaf);
    const float reach = std::fmin(1000.0f, 1000000.0f * leaf);
    for (uint64_t i = 0; i < count / 7; ++i) {
      // key round trip and the single-row identity
      float p[3];
      int32_t c[3];
      bool ok = true;
      for (int a = 0; a < 3; ++a) {
        p[a] = (2.0f * unit(mix(3 * i + a)) - 1.0f) * reach;
        ok = vg::cell_of(p[a], inv, &c[a]) && ok;
      }
      if (!ok) {
        fail("cell_of refused a point inside the range", p[0], leaf);
        continue;
      }
      int32_t d[3];
      vg::cells_of_key(vg::key_of(c[0], c[1], c[2]), &d[0], &d[1], &d[2]);
      if (d[0] != c[0] || d[1] != c[1] || d[2] != c[2]) fail("key round trip", c[0], d[0]);
      for (int a = 0; a < 3; ++a) {
        const int64_t q = vg::fixed_of(p[a]) - vg::corner_of(c[a], leaf);
        const float back = vg::centroid_of(c[a], leaf, q, 1u);
        if (std::fabs(p[a]) >= 0.001953125f ? std::memcmp(&back, &p[a], 4) != 0
                                            : std::fabs(static_cast<double>(back) - static_cast<double>(p[a])) > 1.0 / 8589934592.0)
          fail("single row", p[a], back);
      }
    }
    // centroid of small groups inside one cell against the quotient over the absolute sums (128-bit)
    for (uint64_t g = 0; g < count / 70; ++g) {
      const int32_t c = static_cast<int32_t>(mix(g) % 2001) - 1000;
      const uint32_t n = 1u + static_cast<uint32_t>(mix(g ^ 0x55) % 9);
      int64_t sum_q = 0;
      __int128 sum_abs = 0;
      uint32_t taken = 0;
      for (uint32_t k = 0; k < n; ++k) {
        const float x = (static_cast<float>(c) + unit(mix(g * 16 + k))) * leaf;
        int32_t cc;
        if (!vg::cell_of(x, inv, &cc) || cc != c) continue;  // (rounded across the face: another voxel's row)
        sum_q += vg::fixed_of(x) - vg::corner_of(c, leaf);
        sum_abs += vg::fixed_of(x);
        taken += 1u;
      }
      if (!taken) continue;
      const __int128 num = 2 * sum_abs + taken, den = 2 * static_cast<__int128>(taken);
      __int128 quo = num / den;
      if (num % den < 0) quo -= 1;
      const float want = static_cast<float>(static_cast<double>(static_cast<int64_t>(quo)) * (1.0 / 4294967296.0));
      const float got = vg::centroid_of(c, leaf, sum_q, taken);
      if (std::memcmp(&want, &got, 4) != 0) fail("centroid", want, got);
    }
  }
  // refusals
  int32_t c;
  if (vg::cell_of(NAN, 1000.0f, &c) || vg::cell_of(INFINITY, 1.0f, &c) || vg::cell_of(200.0f, vg::inverse_leaf(1e-4f), &c) ||
      !vg::cell_of(-0.0f, 1000.0f, &c) || c != 0 || !vg::cell_of(-1e-45f, 1000.0f, &c) || c != -1)
    fail("refusals", c, 0);
  std::printf("%llu mismatches\n", static_cast<unsigned long long>(bad));
  return bad ? 1 : 0;
}
