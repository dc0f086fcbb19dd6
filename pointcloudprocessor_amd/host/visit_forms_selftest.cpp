// visit_forms_selftest -- csrc/pcp_visit_forms.hpp compiled for the host (-ffp-contract=off, std::fma): the short forms of the
// distortion, of the cell rule and of the fp32 square root against the written ones, on random and on edge operands.  CPU only:
// the device runs the same text through pcp_selftest_visit_forms().  Exit code 0 iff nothing disagrees.
// usage: visit_forms_selftest [random samples per part]
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/pcp_visit_forms.hpp"

namespace vf = pcp::vf;

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}
static float f32_of(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
static uint32_t bits_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}
static uint64_t bits_of(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}
static bool same(double a, double b) { return (a != a && b != b) || bits_of(a) == bits_of(b); }
static bool same(float a, float b) { return (a != a && b != b) || bits_of(a) == bits_of(b); }

// ---- 1. distortion ------------------------------------------------------------------------------------------------------------
static long check_distortion(long samples) {
  const double inf = INFINITY, nan = NAN;
  const vf::Distortion sets[] = {
      {0.003043514741045163, 0.06634739187544138, 0.0, -0.000217681797407554, -0.0006654964142658197},  // the default camera
      {0.0, 0.0, 0.0, 0.0, 0.0},
      {0.1, -0.02, 0.003, 0.0, 0.0},
      {-0.2, 0.05, -0.001, -0.01, -0.02},
      {0.1, 0.2, 0.3, 0x1p-400, -0x1p400},  // the edges of the tame range
      {1e10, -1e20, 1e30, 1e100, -0.0},
  };
  // what the projection can hand over: quotients of promoted floats (0, +-[2^-277, 2^277]) and non-finite values
  std::vector<double> edge = {0.0, -0.0, inf, -inf, nan, 1.0, -1.0, 0.5, 0x1p-277, -0x1p-277, 0x1p277, -0x1p277,
                              0x1p-149 / 3.0, 3.0e38 / 0x1p-149, 1.0 / 3.0, -2.0 / 3.0, 0x1p128, 0x1p-128};
  long bad = 0, done = 0;
  for (const vf::Distortion &c : sets) {
    if (!vf::distortion_is_tame(c.p1, c.p2)) {
      std::printf("distortion: a coefficient set of the test is not tame\n");
      return 1;
    }
    auto one = [&](double xn, double yn) {
      double xa, ya, xb, yb;
      vf::distort_written(c, xn, yn, xa, ya);
      vf::distort_short(c, xn, yn, xb, yb);
      ++done;
      if (!same(xa, xb) || !same(ya, yb)) {
        if (bad < 10) std::printf("distortion: xn %a yn %a: written (%a, %a) short (%a, %a)\n", xn, yn, xa, ya, xb, yb);
        ++bad;
      }
    };
    for (double a : edge)
      for (double b : edge) one(a, b);
    for (long i = 0; i < samples; ++i) {
      // x / z, y / z of random floats over every exponent (every fourth triple: metre-scale exponents), as the kernels form them
      const uint64_t r = mix(static_cast<uint64_t>(i) * 3u + 17u), s = mix(r);
      uint32_t bx = static_cast<uint32_t>(r), by = static_cast<uint32_t>(r >> 32), bz = static_cast<uint32_t>(s);
      if ((s >> 32) & 3u) {
        bx = (bx & 0x807fffffu) | ((121u + (bx >> 23) % 12u) << 23);
        by = (by & 0x807fffffu) | ((121u + (by >> 23) % 12u) << 23);
        bz = (bz & 0x807fffffu) | ((121u + (bz >> 23) % 12u) << 23);
      }
      const float x = f32_of(bx), y = f32_of(by), z = std::fabs(f32_of(bz));
      if (!(z > 0.0f)) continue;
      one(static_cast<double>(x) / static_cast<double>(z), static_cast<double>(y) / static_cast<double>(z));
    }
  }
  // coefficients outside the tame range are recognised (the kernels then keep the written form)
  const double wild[] = {0x1p-401, -0x1p-401, 0x1p401, 4.9e-324, 1e-200, inf, -inf, nan};
  for (double p : wild)
    if (vf::distortion_is_tame(p, 0.0) || vf::distortion_is_tame(0.0, p) || vf::distortion_is_tame(p, p)) {
      std::printf("distortion: %a passes as tame\n", p);
      ++bad;
    }
  std::printf("distortion: %ld pairs, %ld mismatches\n", done, bad);
  return bad;
}

// ---- 2. cell rule -----------------------------------------------------------------------------------------------------------
static long check_cells(long samples) {
  struct Geometry {
    int32_t cull_w, cull_h, ds;
  };
  const Geometry sets[] = {{703, 405, 14}, {703, 405, 1}, {703, 405, 7}, {703, 405, 20}, {4096, 3000, 14}, {13, 405, 14},
                           {703, 5, 7}, {1 << 24, 100, 1}, {100, 1 << 24, 1}, {(1 << 24) - 1, 3, 2}};
  long bad = 0, done = 0;
  for (const Geometry &g : sets) {
    const int32_t mw = g.cull_w / g.ds, mh = g.cull_h / g.ds;
    const float cwf = static_cast<float>(g.cull_w), chf = static_cast<float>(g.cull_h);
    const float mwf = vf::map_bound(mw), mhf = vf::map_bound(mh);
    std::vector<float> edge = {0.0f, -0.0f, -1.0f, std::nextafter(-1.0f, 0.0f), std::nextafter(-1.0f, -2.0f), -0.5f, 0.5f,
                               1.0f, INFINITY, -INFINITY, NAN, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN, 1e-45f, -1e-45f,
                               2147483648.0f, -2147483648.0f, 4294967296.0f, 16777216.0f};
    for (float m : {static_cast<float>(mw), static_cast<float>(mh), cwf, chf, cwf / static_cast<float>(g.ds), chf / static_cast<float>(g.ds)})
      for (float e : {m, std::nextafter(m, 0.0f), std::nextafter(m, INFINITY), m - 1.0f, m - 0.5f, m + 0.5f}) edge.push_back(e);
    auto one = [&](float qx, float qy) {
      const int32_t a = vf::map_cell_written(qx, qy, cwf, chf, mw, mh);
      int32_t cell = 0;
      const int32_t b = vf::map_cell_short(qx, qy, mwf, mhf, mw, cell) ? cell : -1;
      ++done;
      if (a != b) {
        if (bad < 10) std::printf("cell: %d x %d / %d, q (%a, %a): written %d short %d\n", g.cull_w, g.cull_h, g.ds, qx, qy, a, b);
        ++bad;
      }
    };
    for (float a : edge)
      for (float b : edge) one(a, b);
    for (long i = 0; i < samples; ++i) {
      const uint64_t r = mix(static_cast<uint64_t>(i) * 5u + 3u);
      float qx = f32_of(static_cast<uint32_t>(r)), qy = f32_of(static_cast<uint32_t>(r >> 32));
      if (i & 1) {  // around the map: [-2, 1.25 m)
        qx = (static_cast<float>(static_cast<uint32_t>(r) >> 8) * 0x1p-24f) * (1.25f * cwf + 2.0f) - 2.0f;
        qy = (static_cast<float>(static_cast<uint32_t>(r >> 32) >> 8) * 0x1p-24f) * (1.25f * chf + 2.0f) - 2.0f;
      }
      one(qx, qy);
    }
  }
  std::printf("cell: %ld pairs, %ld mismatches\n", done, bad);
  return bad;
}

// ---- 4. square root ---------------------------------------------------------------------------------------------------------
// every float within 1 ulp of the real root as the estimate: the two floats around it, and for an exact root that root and both
// of its neighbours
static long check_sqrt(long samples) {
  long bad = 0, done = 0;
  auto one = [&](float x) {
    if (!vf::sqrt_in_window(x)) {
      // outside the window the kernels call sqrtf itself: only the window's own test is checked here
      if (x >= 0x1p-96f && x <= FLT_MAX) {
        std::printf("sqrt: %a is in the window but not recognised\n", x);
        ++bad;
      }
      return;
    }
    const float want = std::sqrt(x);  // correctly rounded (IEEE)
    const double root = std::sqrt(static_cast<double>(x));
    float lo = static_cast<float>(root);
    if (static_cast<double>(lo) > root) lo = std::nextafter(lo, 0.0f);
    float cand[3];
    int n = 0;
    if (static_cast<double>(lo) == root) {
      cand[n++] = std::nextafter(lo, 0.0f);
      cand[n++] = lo;
      cand[n++] = std::nextafter(lo, INFINITY);
    } else {
      cand[n++] = lo;
      cand[n++] = std::nextafter(lo, INFINITY);
    }
    for (int k = 0; k < n; ++k) {
      const float got = vf::sqrt_from_estimate(x, cand[k]);
      ++done;
      if (!same(got, want)) {
        if (bad < 10) std::printf("sqrt: x %a estimate %a: %a, sqrtf %a\n", x, cand[k], got, want);
        ++bad;
      }
    }
  };
  const float edge[] = {0.0f, -0.0f, -1.0f, INFINITY, -INFINITY, NAN, 1e-45f, FLT_MIN, std::nextafter(0x1p-96f, 0.0f), 0x1p-96f,
                        std::nextafter(0x1p-96f, 1.0f), 0x1p-95f, FLT_MAX, std::nextafter(FLT_MAX, 0.0f), 1.0f, 2.0f, 4.0f,
                        std::nextafter(1.0f, 0.0f), std::nextafter(1.0f, 2.0f), std::nextafter(4.0f, 0.0f), 0x1p127f, 0x1p126f};
  for (float x : edge) one(x);
  for (int e = -96; e <= 127; ++e) {  // the first and last floats of every binade and its exact squares' neighbourhood
    const float p = std::ldexp(1.0f, e);
    for (float x : {p, std::nextafter(p, INFINITY), std::nextafter(p, 0.0f), p * 1.5f, p * 1.5625f}) one(x);
  }
  for (uint32_t k = 1; k < 4096; ++k) {  // exact squares and their neighbours
    const float s = static_cast<float>(k) * static_cast<float>(k);
    one(s);
    one(std::nextafter(s, 0.0f));
    one(std::nextafter(s, INFINITY));
  }
  for (long i = 0; i < samples; ++i) one(f32_of(static_cast<uint32_t>(mix(static_cast<uint64_t>(i) * 7u + 1u))));
  std::printf("sqrt: %ld estimates, %ld mismatches\n", done, bad);
  return bad;
}

int main(int argc, char **argv) {
  const long samples = argc > 1 ? std::atol(argv[1]) : 1000000;
  const long bad = check_distortion(samples) + check_cells(samples) + check_sqrt(samples);
  std::printf("visit_forms_selftest: %ld mismatches\n", bad);
  return bad == 0 ? 0 : 1;
}
