// compare_selftest -- csrc/pcp_compare.hpp compiled for the host (CPU only: never a GPU job; meant to be built with
// -fsanitize=address,undefined as well).  Checks the parameters' bounds, the quantisation of the normal (ties to even), the
// orientation modes, the axial and radial boundary of the integer cylinder, the sphere test that comes before it, the ranges of
// MC3 at the widest search radius against 128-bit arithmetic, the sums against 128-bit sums and their invariance under the
// order of the candidates, and the status byte's order of tests.  Prints the number of mismatches; exit code 0 iff none.
//   usage: compare_selftest [points]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/pcp_compare.hpp"

using namespace pcp;

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

static float unit(uint64_t r) { return static_cast<float>(static_cast<double>(r >> 11) * (1.0 / 9007199254740992.0)); }

int main(int argc, char **argv) {
  const int64_t count = argc > 1 ? std::strtoll(argv[1], nullptr, 10) : 1500;
  uint64_t bad = 0;
  auto fail = [&](const char *what, double a, double b) {
    if (bad < 10) std::fprintf(stderr, "mismatch (%s): %.17g %.17g\n", what, a, b);
    ++bad;
  };
  const float none[3] = {0.0f, 0.0f, 0.0f};
  mc::Rule r;
  // MC3 / MC6: the bounds
  if (mc::prepare(0.03f, 0.05f, 0.0f, 5, 0, none, &r) != nullptr) fail("defaults refused", 0, 0);
  if (mc::prepare(0.005f, 0.005f, 0.0f, 2, 0, none, &r) != nullptr) fail("lower bounds refused", 0, 0);
  if (!mc::prepare(std::nextafter(0.005f, 0.0f), 0.05f, 0.0f, 5, 0, none, &r)) fail("cyl_radius below the bound taken", 0, 0);
  if (!mc::prepare(0.03f, std::nextafter(0.005f, 0.0f), 0.0f, 5, 0, none, &r)) fail("cyl_half_length below the bound taken", 0, 0);
  if (!mc::prepare(0.3f, 0.4f, 0.0f, 5, 0, none, &r)) fail("search radius above 0.5 taken", 0, 0);
  if (!mc::prepare(NAN, 0.05f, 0.0f, 5, 0, none, &r) || !mc::prepare(0.03f, INFINITY, 0.0f, 5, 0, none, &r)) fail("non-finite extent taken", 0, 0);
  if (!mc::prepare(0.03f, 0.05f, -1e-9f, 5, 0, none, &r) || !mc::prepare(0.03f, 0.05f, NAN, 5, 0, none, &r)) fail("reg_error taken", 0, 0);
  if (!mc::prepare(0.03f, 0.05f, 0.0f, 1, 0, none, &r)) fail("min_points 1 taken", 0, 0);
  if (!mc::prepare(0.03f, 0.05f, 0.0f, 5, 3, none, &r) || !mc::prepare(0.03f, 0.05f, 0.0f, 5, -1, none, &r)) fail("orient_mode taken", 0, 0);
  {
    const float nan3[3] = {NAN, 0.0f, 0.0f};
    if (!mc::prepare(0.03f, 0.05f, 0.0f, 5, 1, nan3, &r)) fail("non-finite orient taken", 0, 0);
  }
  // the widest rule: L the largest float that keeps the search radius at 0.5
  float wide_l = 0.4f;
  while (mc::prepare(0.3f, wide_l, 0.0f, 5, 0, none, &r)) wide_l = std::nextafter(wide_l, 0.0f);
  if (r.search_radius != 0.5f || r.t != 0.25f) fail("widest search radius", r.search_radius, r.t);
  const mc::Rule wide = r;

  // MC2: the normal's quanta, ties to even
  if (mc::quantise_normal(0.6f) != 1229 || mc::quantise_normal(-0.6f) != -1229 || mc::quantise_normal(0.5f / 2048.0f) != 0 ||
      mc::quantise_normal(1.5f / 2048.0f) != 2 || mc::quantise_normal(-2.5f / 2048.0f) != -2 || mc::quantise_normal(1.0f) != 2048)
    fail("quantise_normal", 0, 0);
  mc::Direction d;
  if (mc::prepare(0.03f, 0.05f, 0.0f, 5, 0, none, &r)) fail("defaults", 0, 0);
  if (mc::direction(r, 0, 0, 0, 0.0f, 0.0f, 0.0f, d) || mc::direction(r, 0, 0, 0, NAN, 0.0f, 1.0f, d) ||
      mc::direction(r, 0, 0, 0, 0.0f, 1.5f, 0.0f, d) || mc::direction(r, 0, 0, 0, 0.0002f, 0.0001f, 0.0f, d))
    fail("an invalid normal made a core point", 0, 0);
  if (!mc::direction(r, 0, 0, 0, 0.0f, 0.0f, -1.0f, d) || d.N[2] != -2048 || d.N2 != 4194304) fail("mode 0 keeps the sign", d.N[2], 0);
  {
    const float up[3] = {1.0f, 2.0f, 9.0f};
    mc::Rule r1, r2;
    if (mc::prepare(0.03f, 0.05f, 0.0f, 5, 1, up, &r1) || mc::prepare(0.03f, 0.05f, 0.0f, 5, 2, up, &r2)) fail("modes 1, 2", 0, 0);
    // the point (1, 2, 10) lies above `up`: mode 1 turns (0, 0, 1) down, mode 2 (along +z) keeps it
    if (!mc::direction(r1, 1.0f, 2.0f, 10.0f, 0.0f, 0.0f, 1.0f, d) || d.N[2] != -2048) fail("mode 1", d.N[2], 0);
    if (!mc::direction(r2, 1.0f, 2.0f, 10.0f, 0.0f, 0.0f, 1.0f, d) || d.N[2] != 2048) fail("mode 2", d.N[2], 0);
    if (!mc::direction(r2, 1.0f, 2.0f, 10.0f, 0.0f, 0.0f, -1.0f, d) || d.N[2] != 2048) fail("mode 2 flips", d.N[2], 0);
  }

  // MC3: the boundary of the integer cylinder, normal (0, 0, 1), rc = 32765 quanta = 5 * 6553, L = 0.05
  {
    const float q = 1.0f / 1048576.0f;
    if (mc::prepare(32765.0f * q, 0.05f, 0.0f, 2, 0, none, &r)) fail("boundary rule", 0, 0);
    if (r.rc2 != int64_t(32765) * 32765) fail("rc2", static_cast<double>(r.rc2), 0);
    if (!(int64_t(52428) * 52428 <= r.L2 && r.L2 < int64_t(52429) * 52429)) fail("L2", static_cast<double>(r.L2), 0);
    if (!mc::direction(r, 0, 0, 0, 0.0f, 0.0f, 1.0f, d)) fail("boundary direction", 0, 0);
    struct Case {
      int32_t x, y, z;
      bool in;
    };
    const Case cases[] = {{0, 0, 52428, true},      {0, 0, 52429, false},      {0, 0, -52428, true},     {0, 0, -52429, false},
                          {19659, 26212, 0, true},  {19659, 26213, 0, false},  {-19659, -26212, 9, true}, {-19660, -26212, 0, false},
                          {32765, 0, -40000, true}, {32766, 0, 0, false},      {0, 0, 0, true}};
    for (const Case &c : cases) {
      int64_t h;
      if (mc::in_cylinder(d, c.x, c.y, c.z, h) != c.in) fail("in_cylinder", c.x, c.z);
      mc::Sums s;
      mc::clear(s);
      // whole quanta below 2^24 are exact floats, and all of these lie inside the sphere
      if (mc::visit(s, d, r.t, c.x * q, c.y * q, c.z * q, 1) != c.in) fail("visit", c.x, c.z);
      if (s.nB != (c.in ? 1 : 0) || s.nA != 0 || s.s1B != (c.in ? int64_t(c.z) * 2048 : 0)) fail("visit sums", c.x, c.z);
    }
    // the sphere comes first: with L a whole number of quanta, an offset that quantises to the cylinder's corner from outside
    if (mc::prepare(32765.0f * q, 52428.0f * q, 0.0f, 2, 0, none, &r)) fail("corner rule", 0, 0);
    if (!mc::direction(r, 0, 0, 0, 0.0f, 0.0f, 1.0f, d)) fail("corner direction", 0, 0);
    const float cx = 32765.4f * q, cz = 52428.4f * q;
    int64_t h;
    mc::Sums s;
    mc::clear(s);
    if (!mc::in_cylinder(d, gn::quantise(cx), 0, gn::quantise(cz), h)) fail("the corner's quanta are inside", 0, 0);
    if (mc::visit(s, d, r.t, cx, 0.0f, cz, 0) || s.nA != 0) fail("outside the sphere, yet taken", 0, 0);
    if (!mc::visit(s, d, r.t, 32765.0f * q, 0.0f, 52428.0f * q, 0) || s.nA != 1) fail("the corner itself", 0, 0);
  }

  // MC3's ranges at the widest rule, offsets out to the rim, unit and longest normals; MC4 against 128-bit sums
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<float> off(static_cast<size_t>(3 * count));
    for (int64_t k = 0; k < 3 * count; ++k) off[static_cast<size_t>(k)] = (2.0f * unit(mix(77 + static_cast<uint64_t>(k))) - 1.0f) * 0.5f;
    for (int64_t i = 0; i < 64; ++i) {
      float nx = 2.0f * unit(mix(900 + 3 * static_cast<uint64_t>(i))) - 1.0f, ny = 2.0f * unit(mix(901 + 3 * static_cast<uint64_t>(i))) - 1.0f,
            nz = 2.0f * unit(mix(902 + 3 * static_cast<uint64_t>(i))) - 1.0f;
      if (pass == 0) {
        const float len = std::sqrt(nx * nx + ny * ny + nz * nz);
        nx /= len, ny /= len, nz /= len;
      } else if (i == 0) {
        nx = ny = nz = 1.0f;  // the longest normal the rule admits
      }
      if (!mc::direction(wide, 0, 0, 0, nx, ny, nz, d)) continue;
      mc::Sums fwd, bwd;
      mc::clear(fwd);
      mc::clear(bwd);
      __int128 want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int64_t k = 0; k < count; ++k) {
        const float *o = &off[static_cast<size_t>(3 * k)];
        const uint32_t epoch = static_cast<uint32_t>(k & 1);
        const float d2 = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
        if (d2 <= wide.t && !mc::bounds_hold(wide, d, gn::quantise(o[0]), gn::quantise(o[1]), gn::quantise(o[2])))
          fail("ranges", o[0], o[2]);
        if (mc::visit(fwd, d, wide.t, o[0], o[1], o[2], epoch)) {
          const __int128 h = static_cast<__int128>(gn::quantise(o[0])) * d.N[0] + static_cast<__int128>(gn::quantise(o[1])) * d.N[1] +
                             static_cast<__int128>(gn::quantise(o[2])) * d.N[2];
          const __int128 hh = h * h;
          __int128 *w = want + 4 * epoch;
          w[0] += 1, w[1] += h, w[2] += hh & 0xffffffff, w[3] += hh >> 32;
        }
      }
      for (int64_t k = count - 1; k >= 0; --k) {
        const float *o = &off[static_cast<size_t>(3 * k)];
        mc::visit(bwd, d, wide.t, o[0], o[1], o[2], static_cast<uint32_t>(k & 1));
      }
      int64_t a_[8], b_[8];
      mc::store(fwd, a_);
      mc::store(bwd, b_);
      if (std::memcmp(a_, b_, sizeof(a_)) != 0) fail("order of the candidates", static_cast<double>(i), 0);
      for (int a = 0; a < 8; ++a)
        if (static_cast<__int128>(a_[a]) != want[a]) fail("sums", static_cast<double>(a_[a]), static_cast<double>(want[a]));
    }
  }

  // MC5 / MC6: the order of the tests, the sign, and the three operations of the distance written out
  {
    if (mc::prepare(0.03f, 0.05f, 0.0f, 5, 0, none, &r)) fail("defaults", 0, 0);
    if (!mc::direction(r, 0, 0, 0, 0.6f, 0.0f, 0.8f, d)) fail("finish direction", 0, 0);
    mc::Sums s;
    mc::clear(s);
    s.nA = 4, s.nB = 4;
    if (mc::finish(r, d, s).status != mc::kNoCounterpart) fail("nB is tested first", 0, 0);
    s.nB = 5;
    if (mc::finish(r, d, s).status != mc::kTooFewOwn) fail("nA second", 0, 0);
    s.nA = 5;
    mc::Result z = mc::finish(r, d, s);
    if (z.status != mc::kMeasured || z.distance != 0.0f || z.lod != 0.0f) fail("all zero", z.distance, z.lod);
    s.s1A = 5 * 7000, s.s2aA = 5 * int64_t(7000) * 7000;  // five candidates at h = 7000 (S2b stays 0), the base at 0
    z = mc::finish(r, d, s);
    const volatile double scale = std::sqrt(static_cast<double>(d.N2)) * 1048576.0;
    const volatile double mean = 35000.0 / 5.0 - 0.0 / 5.0;
    const float want = static_cast<float>(mean / scale);
    if (z.status != mc::kPositive || std::memcmp(&want, &z.distance, 4) != 0 || z.lod != 0.0f) fail("positive", z.distance, want);
    s.s1A = -s.s1A;
    z = mc::finish(r, d, s);
    if (z.status != mc::kNegative || z.distance != -want) fail("negative", z.distance, want);
    mc::Rule reg;
    if (mc::prepare(0.03f, 0.05f, 0.01f, 5, 0, none, &reg)) fail("reg rule", 0, 0);
    z = mc::finish(reg, d, s);
    if (z.status != mc::kMeasured || z.lod != 0.01f) fail("reg_error raises the level", z.lod, 0);
    // a variance that rounds below zero is zero: equal h whose S1 * S1 / n rounds above S2
    if (mc::variance(3, 3 * int64_t(94906267), (3 * (int64_t(94906267) * 94906267)) & 0xffffffff, (3 * (int64_t(94906267) * 94906267)) >> 32) < 0.0)
      fail("negative variance", 0, 0);
  }
  std::printf("%llu mismatches\n", static_cast<unsigned long long>(bad));
  return bad ? 1 : 0;
}
