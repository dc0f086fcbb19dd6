// ortho_cyl_selftest -- csrc/pcp_ortho_cyl.hpp compiled for the host (CPU only: never a GPU job).  Checks CY3's angle on the
// octant boundaries, on both sides of tan(pi/8), on the signed zeros and against atan2 within 1e-9 rad; CY2 at the seam, at the
// raster's borders, on the axis and at the depth window's ends for both sides; the frame rules of CY1; and a tiny unrolled map
// worked out by hand.  Prints the number of mismatches; exit code 0 iff none.   usage: ortho_cyl_selftest [count]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/pcp_ortho_cyl.hpp"

using namespace pcp;

static int bad = 0;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("line %d: %s\n", __LINE__, #cond);         \
      ++bad;                                                 \
    }                                                        \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double rnd() {  // in (-1, 1)
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return static_cast<double>(static_cast<int64_t>(rng_state >> 11) - (int64_t(1) << 52)) / static_cast<double>(int64_t(1) << 52);
}

// the cylinder about the z axis through the origin: theta from +x towards side * y, rows run down -z from z = top
static cy::Frame upright(float radius, int32_t side, int32_t w, int32_t h, float gsd, float top, float d_min, float d_max) {
  cy::Frame f{};
  f.c[2] = top;
  f.a[2] = -1.0f;
  f.e[0] = 1.0f;
  f.b[1] = side > 0 ? -1.0f : 1.0f;  // b = side (a x e), a x e = (0, -1, 0)
  f.inv = om::inverse_gsd(gsd);
  f.w = w;
  f.h = h;
  f.wf = static_cast<float>(w);
  f.hf = static_cast<float>(h);
  f.d_min = d_min;
  f.d_max = d_max;
  f.R = static_cast<double>(radius);
  f.side = static_cast<double>(side);
  return f;
}

static double wrap_error(double got, double s, double t) {
  double want = std::atan2(t, s);
  if (want < 0.0) want += cy::kTwoPi;
  double d = std::fabs(got - want);
  return std::fmin(d, cy::kTwoPi - d);
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? std::atoi(argv[1]) : 200000;

  // CY3: exact values on the axes and the diagonals, the signed zeros, the range
  EXPECT(cy::angle(1.0, 0.0) == 0.0 && cy::angle(1.0, -0.0) == 0.0);  // -0 is not < 0
  EXPECT(cy::angle(0.0, 1.0) == cy::kPi2 && cy::angle(-0.0, 1.0) == cy::kPi2);
  EXPECT(cy::angle(-1.0, 0.0) == cy::kPi && cy::angle(-1.0, -0.0) == cy::kPi);
  EXPECT(cy::angle(0.0, -1.0) == cy::kTwoPi - cy::kPi2);
  EXPECT(cy::angle(3.0, 3.0) == cy::kPi4 && cy::angle(-3.0, 3.0) == cy::kPi - cy::kPi4);
  EXPECT(cy::angle(-3.0, -3.0) == cy::kTwoPi - (cy::kPi - cy::kPi4) && cy::angle(3.0, -3.0) == cy::kTwoPi - cy::kPi4);
  EXPECT(cy::angle(1.0, -4.9e-324) == cy::kTwoPi);  // the quotient underflows: 2 pi, not wrapped
  EXPECT(cy::angle(0.0, 0.0) != cy::angle(0.0, 0.0));  // NaN: CY2 never asks
  {
    const double below = std::nextafter(cy::kTan8, 0.0), above = std::nextafter(cy::kTan8, 1.0);
    for (const double q : {below, cy::kTan8, above}) {
      EXPECT(wrap_error(cy::angle(1.0, q), 1.0, q) <= 1e-9 && wrap_error(cy::angle(q, 1.0), q, 1.0) <= 1e-9);
      EXPECT(wrap_error(cy::angle(-1.0, -q), -1.0, -q) <= 1e-9);
    }
    // (the two branches meet within twice the series' truncation bound, t8^27 / 27 = 1.7e-12 rad each)
    EXPECT(cy::angle(1.0, below) <= cy::angle(1.0, cy::kTan8) && cy::angle(1.0, cy::kTan8) <= cy::angle(1.0, above) + 4e-12);
  }
  double worst = 0.0;
  for (int i = 0; i < count; ++i) {
    const double scale = i % 3 == 0 ? 1e-3 : (i % 3 == 1 ? 1.0 : 1e3);
    const double s = rnd() * scale, t = rnd() * scale;
    if (s == 0.0 && t == 0.0) continue;
    const double th = cy::angle(s, t);
    EXPECT(th >= 0.0 && th <= cy::kTwoPi);
    worst = std::fmax(worst, wrap_error(th, s, t));
  }
  EXPECT(worst <= 1e-9);

  // CY2 on a cylinder of R = 1 seen from outside: 8 x 4 pixels of 0.25 m, window [-0.5, 0.5], top at z = 1
  {
    const cy::Frame f = upright(1.0f, -1, 8, 4, 0.25f, 1.0f, -0.5f, 0.5f);
    int32_t px = -1;
    uint32_t db = 1;
    EXPECT(cy::project(f, 1.0f, 0.0f, 1.0f, &px, &db) && px == 0 && db == 0u);         // theta = 0, h = 0, on the cylinder
    EXPECT(cy::project(f, 0.0f, 1.0f, 1.0f, &px, &db) && px == 6);                     // theta = pi/2: arc 1.5708 m, column 6
    EXPECT(!cy::project(f, -1.0f, 0.0f, 1.0f, &px, &db));                              // theta = pi: column 12, outside
    EXPECT(!cy::project(f, 1.0f, -1e-3f, 1.0f, &px, &db));                             // just before the seam: near 2 pi
    EXPECT(!cy::project(f, 1.0f, 0.0f, 1.0001f, &px, &db));                            // y < 0
    EXPECT(cy::project(f, 1.0f, 0.0f, 0.0001f, &px, &db) && px == 3 * 8);              // the last row
    EXPECT(!cy::project(f, 1.0f, 0.0f, 0.0f, &px, &db));                               // y == H
    EXPECT(!cy::project(f, 0.0f, 0.0f, 0.5f, &px, &db));                               // on the axis
    EXPECT(cy::project(f, 1.5f, 0.0f, 0.5f, &px, &db) && om::bits_float(db) == -0.5f);  // from outside: farther out is nearer
    EXPECT(cy::project(f, 0.5f, 0.0f, 0.5f, &px, &db) && om::bits_float(db) == 0.5f);
    EXPECT(!cy::project(f, 1.5000001f, 0.0f, 0.5f, &px, &db) && !cy::project(f, 0.4999999f, 0.0f, 0.5f, &px, &db));
    const float inf = om::bits_float(0x7f800000u), nan = om::bits_float(0x7fc00000u);
    EXPECT(!cy::project(f, nan, 0.0f, 0.5f, &px, &db) && !cy::project(f, 1.0f, inf, 0.5f, &px, &db) &&
           !cy::project(f, 1.0f, 0.0f, -inf, &px, &db));
    EXPECT(!cy::project(f, 3e38f, 3e38f, 0.5f, &px, &db));                             // rho overflows: outside the window
    // seen from inside the angle runs the other way round and the depth grows outward
    const cy::Frame g = upright(1.0f, 1, 8, 4, 0.25f, 1.0f, -0.5f, 0.5f);
    EXPECT(cy::project(g, 0.0f, -1.0f, 1.0f, &px, &db) && px == 6);
    EXPECT(!cy::project(g, 0.0f, 1.0f, 1.0f, &px, &db));
    EXPECT(cy::project(g, 1.5f, 0.0f, 0.5f, &px, &db) && om::bits_float(db) == 0.5f);
  }

  // CY1
  {
    const float c[3] = {0, 0, 0}, a[3] = {0, 0, -1}, e[3] = {1, 0, 0}, out[3] = {0, 1, 0}, in[3] = {0, -1, 0}, skew[3] = {0.999f, 0.05f, 0};
    const char *why = nullptr;
    double fit = 0.0;
    EXPECT(cy::frame_check(c, a, e, out, 1.0f, 0.01f, 100, 100, -1.0f, 1.0f, -1, &why, &fit) == 0);
    EXPECT(cy::frame_check(c, a, e, in, 1.0f, 0.01f, 100, 100, -1.0f, 1.0f, 1, &why, &fit) == 0);
    EXPECT(cy::frame_check(c, a, e, in, 1.0f, 0.01f, 100, 100, -1.0f, 1.0f, -1, &why, &fit) == 1);  // mirrored for this side
    EXPECT(cy::frame_check(c, a, e, out, 1.0f, 0.01f, 100, 100, -1.0f, 1.0f, 1, &why, &fit) == 1);
    EXPECT(cy::frame_check(c, a, skew, out, 1.0f, 0.01f, 100, 100, -1.0f, 1.0f, -1, &why, &fit) == 1);
    EXPECT(cy::frame_check(c, a, e, out, 1.0f, 0.01f, 100, 100, -1.0f, 1.0f, 0, &why, &fit) == 1);
    EXPECT(cy::frame_check(c, a, e, out, 1.0f, 0.01f, 100, 100, -1.0f, 1.0f, 2, &why, &fit) == 1);
    EXPECT(cy::frame_check(c, a, e, out, 0.04f, 0.01f, 10, 100, -1.0f, 1.0f, -1, &why, &fit) == 1);
    EXPECT(cy::frame_check(c, a, e, out, 1001.0f, 0.01f, 100, 100, -1.0f, 1.0f, -1, &why, &fit) == 1);
    EXPECT(cy::frame_check(c, a, e, out, 1.0f, 2.0f, 1, 1, -1.0f, 1.0f, -1, &why, &fit) == 1);
    EXPECT(cy::frame_check(c, a, e, out, 1.0f, 0.01f, 100, 100, 1.0f, 1.0f, -1, &why, &fit) == 1);
    EXPECT(cy::frame_check(c, a, e, out, 1.0f, 0.01f, 0, 100, -1.0f, 1.0f, -1, &why, &fit) == 1);
    EXPECT(cy::frame_check(c, a, e, out, 1.0f, 0.01f, 629, 100, -1.0f, 1.0f, -1, &why, &fit) == 0);  // 6.29 <= 2 pi + 0.01
    EXPECT(cy::frame_check(c, a, e, out, 1.0f, 0.01f, 630, 100, -1.0f, 1.0f, -1, &why, &fit) == 1);  // wider than the ring
    EXPECT(cy::frame_check(c, a, e, out, 100.0f, 0.01f, 20000, 100, -1.0f, 1.0f, -1, &why, &fit) == 2 && fit > 0.0122 && fit < 0.01222);
    EXPECT(cy::frame_check(c, a, e, out, 100.0f, 0.01f, 16384, 4096, -1.0f, 1.0f, -1, &why, &fit) == 0);
  }

  // a map of 8 x 2 pixels of 0.25 m by hand, seen from outside: rows under the global indices 10 + row
  {
    const cy::Frame f = upright(1.0f, -1, 8, 2, 0.25f, 0.5f, -0.5f, 0.5f);
    const float pts[][3] = {
        {1.0f, 0.1f, 0.4f},    // row 0: pixel 0, on the cylinder within rounding
        {1.2f, 0.12f, 0.4f},   // row 1: pixel 0, 0.2 m farther out: nearer to the viewer outside, wins
        {1.2f, 0.12f, 0.45f},  // row 2: pixel 0, the same depth: a tie, the higher index loses
        {0.0f, 0.9f, 0.1f},    // row 3: pixel 8 + 6
        {0.0f, 0.0f, 0.4f},    // row 4: on the axis
        {-1.0f, 0.1f, 0.4f},   // row 5: past the raster
        {1.6f, 0.0f, 0.4f},    // row 6: outside the window
    };
    std::vector<unsigned long long> keys(16, om::kEmptyKey);
    int contributors = 0;
    for (uint32_t i = 0; i < 7; ++i) {
      int32_t px;
      uint32_t db;
      if (!cy::project(f, pts[i][0], pts[i][1], pts[i][2], &px, &db)) continue;
      ++contributors;
      const unsigned long long k = om::key_of(db, 10u + i);
      if (k < keys[static_cast<size_t>(px)]) keys[static_cast<size_t>(px)] = k;
    }
    EXPECT(contributors == 4);
    EXPECT(om::key_index(keys[0]) == 11u && om::key_depth(keys[0]) < -0.2f && om::key_depth(keys[0]) > -0.21f);
    EXPECT(om::key_index(keys[14]) == 13u && om::key_depth(keys[14]) > 0.09f && om::key_depth(keys[14]) < 0.11f);
    for (int p = 1; p < 16; ++p)
      if (p != 14) EXPECT(keys[static_cast<size_t>(p)] == om::kEmptyKey);
  }

  std::printf("%d mismatches\n", bad);
  return bad ? 1 : 0;
}
