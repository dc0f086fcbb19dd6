// ortho_cyl_texture_selftest -- the way back of csrc/pcp_ortho_cyl.hpp compiled for the host (CPU only: never a GPU job;
// DESIGN.md "Orthophotos of unrolled maps", CT1, CT2, CT7).  Checks CT1's sine and cosine against the C library within 1e-12 and
// the Pythagorean identity within 4e-16 (in long double) on every multiple of pi/4 up to 2 pi and its neighbours, on the angles
// where the quadrant changes and their neighbours, on 0, on the smallest subnormal and on random angles up to 2 pi + 20; the
// quadrants' exact values; CT2 over a fixed frame of 24 x 6 pixels for both sides at k = 1, 2, 3, 16 by a checksum of every
// bit (the expected values come from the numpy restatement tests/_ortho_cyl_texture_ref.py), a point through CY2 and back, and
// rho <= 0.  Prints the number of mismatches; exit code 0 iff none.   usage: ortho_cyl_texture_selftest [count]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/pcp_ortho_cyl.hpp"
#include "../csrc/pcp_ortho_texture.hpp"

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
static double rnd01() {  // in [0, 1)
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return static_cast<double>(rng_state >> 11) / static_cast<double>(uint64_t(1) << 53);
}

static double worst_error = 0.0, worst_identity = 0.0;
static void check_angle(double theta) {
  double s, c;
  cy::sincos(theta, &s, &c);
  const double es = std::fabs(s - std::sin(theta)), ec = std::fabs(c - std::cos(theta));
  const long double ls = s, lc = c;
  const double id = static_cast<double>(fabsl(ls * ls + lc * lc - 1.0L));
  worst_error = std::fmax(worst_error, std::fmax(es, ec));
  worst_identity = std::fmax(worst_identity, id);
  if (!(es <= 1e-12 && ec <= 1e-12 && id <= 4e-16)) {
    std::printf("theta %a: sin off by %g, cos off by %g, identity off by %g\n", theta, es, ec, id);
    ++bad;
  }
}
static void check_about(double theta) {
  check_angle(theta);
  check_angle(std::nextafter(theta, 64.0));
  if (theta > 0.0) check_angle(std::nextafter(theta, 0.0));
}

// the fixed frame of the checksum: the axis down -z through (3, -2, 1), theta = 0 along (0.6, 0.8, 0), b = side (a x e)
static cy::Frame fixed_frame(int32_t side) {
  cy::Frame f{};
  f.c[0] = 3.0f; f.c[1] = -2.0f; f.c[2] = 1.0f;
  f.a[2] = -1.0f;
  f.e[0] = 0.6f; f.e[1] = 0.8f;
  f.b[0] = side > 0 ? 0.8f : -0.8f; f.b[1] = side > 0 ? -0.6f : 0.6f;
  f.inv = om::inverse_gsd(0.01f);
  f.w = 24;
  f.h = 6;
  f.wf = 24.0f;
  f.hf = 6.0f;
  f.d_min = -1.0f;
  f.d_max = 1.0f;
  f.R = static_cast<double>(0.75f);
  f.side = static_cast<double>(side);
  return f;
}

static uint64_t checksum(int32_t side, int32_t k) {
  const cy::Frame f = fixed_frame(side);
  const int32_t W = f.w, H = f.h;
  std::vector<int32_t> source(static_cast<size_t>(W * H));
  std::vector<float> depth(static_cast<size_t>(W * H));
  for (int32_t q = 0; q < W * H; ++q) {
    source[static_cast<size_t>(q)] = q % 7 == 3 ? -1 : (q % 11 == 5 ? q - 1 : q);  // empty pixels, and pixels filled from their left
    depth[static_cast<size_t>(q)] = static_cast<float>((q * 37) % 101 - 50) * 0.001f;
  }
  const ot::Raster r{k, 0, 0, W, H, 1, 0.03f};
  uint64_t h = 0xcbf29ce484222325ull;
  auto mix = [&](uint32_t w) { h = (h ^ w) * 0x100000001b3ull; };
  for (int32_t Y = 0; Y < H * k; ++Y)
    for (int32_t X = 0; X < W * k; ++X) {
      float d = 0.0f, p[3] = {0.0f, 0.0f, 0.0f};
      bool ok = ot::surface_depth(r, W, H, source.data(), [&](int32_t s) { return depth[static_cast<size_t>(s)]; }, X, Y, &d);
      if (ok) ok = cy::surface_point(f, k, X, Y, d, p);
      mix(ok ? 1u : 0u);
      for (int a = 0; a < 3; ++a) mix(om::float_bits(p[a]));
    }
  return h;
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? std::atoi(argv[1]) : 200000;

  // CT1: the listed angles
  for (int j = 0; j <= 8; ++j) check_about(static_cast<double>(j) * cy::kPi4);
  check_angle(0.0);
  check_angle(4.9e-324);
  for (int m = 0; m < 17; ++m) {  // where theta (2 / pi) + 0.5 crosses an integer: k changes between two neighbours
    double t = (static_cast<double>(m) + 0.5) / cy::kTwoOverPi;
    for (int i = 0; i < 8 && static_cast<int>(t * cy::kTwoOverPi + 0.5) > m; ++i) t = std::nextafter(t, 0.0);
    while (static_cast<int>(std::nextafter(t, 64.0) * cy::kTwoOverPi + 0.5) == m) t = std::nextafter(t, 64.0);
    EXPECT(static_cast<int>(t * cy::kTwoOverPi + 0.5) == m && static_cast<int>(std::nextafter(t, 64.0) * cy::kTwoOverPi + 0.5) == m + 1);
    check_about(t);
    check_about(std::nextafter(t, 64.0));
  }
  for (int i = 0; i < count; ++i) check_angle((i % 4 ? cy::kTwoPi : cy::kTwoPi + 20.0) * rnd01());
  {
    double s, c;
    cy::sincos(0.0, &s, &c);
    EXPECT(s == 0.0 && c == 1.0);
    cy::sincos(4.9e-324, &s, &c);
    EXPECT(s == 4.9e-324 && c == 1.0);
    cy::sincos(cy::kPi2, &s, &c);  // r = 0 in every quadrant: the exact values, signed zeros aside
    EXPECT(s == 1.0 && c == 0.0);
    cy::sincos(cy::kPi, &s, &c);
    EXPECT(s == 0.0 && c == -1.0);
    cy::sincos(3.0 * cy::kPi2, &s, &c);
    EXPECT(s == -1.0 && c == 0.0);
    cy::sincos(cy::kTwoPi, &s, &c);
    EXPECT(s == 0.0 && c == 1.0);
  }
  std::printf("sincos: worst error %g, worst |s^2 + c^2 - 1| %g\n", worst_error, worst_identity);

  // CT2: every bit over the fixed frame
  static const struct {
    int32_t side, k;
    uint64_t want;
  } sums[] = {
      {1, 1, 0x2061283a8a734d60ull}, {1, 2, 0xca59c1374da333ebull}, {1, 3, 0x6a20a58fd97fed3dull}, {1, 16, 0x297f306d60e9fc0cull},
      {-1, 1, 0xaf0471e3366949fdull}, {-1, 2, 0xbfacd12fef3af81bull}, {-1, 3, 0xd818fd1b9098eb5dull}, {-1, 16, 0x640eb3ffa82891d0ull},
  };
  for (const auto &e : sums) {
    const uint64_t got = checksum(e.side, e.k);
    if (got != e.want) {
      std::printf("side %d, k %d: checksum 0x%016" PRIx64 ", expected 0x%016" PRIx64 "\n", e.side, e.k, got, e.want);
      ++bad;
    }
  }

  // CT2 against CY2: the centre of a pixel at depth d comes back to that pixel and that depth; rho <= 0 is no surface
  for (const int32_t side : {1, -1}) {
    const cy::Frame f = fixed_frame(side);
    for (int32_t k : {1, 2, 3, 16})
      for (int32_t Y = 0; Y < f.h * k; Y += 5)
        for (int32_t X = 0; X < f.w * k; X += 7) {
          const float d = 0.001f * static_cast<float>((X + 3 * Y) % 41 - 20);
          float p[3], x, y, back;
          EXPECT(cy::surface_point(f, k, X, Y, d, p));
          EXPECT(cy::coords(f, p[0], p[1], p[2], &x, &y, &back));
          EXPECT(static_cast<int32_t>(floorf(x)) == X / k && static_cast<int32_t>(floorf(y)) == Y / k && std::fabs(back - d) <= 1e-5f);
        }
    float p[3] = {7.0f, 7.0f, 7.0f};
    EXPECT(!cy::surface_point(f, 1, 0, 0, side > 0 ? -0.75f : 0.75f, p) && p[0] == 7.0f);  // rho == 0
    EXPECT(!cy::surface_point(f, 1, 0, 0, side > 0 ? -1.0f : 1.0f, p));                      // rho < 0
    EXPECT(!cy::surface_point(f, 1, 0, 0, om::bits_float(0x7fc00000u), p));                  // a NaN depth: rho > 0 is false
    EXPECT(cy::surface_point(f, 1, 0, 0, side > 0 ? -0.74f : 0.74f, p));
  }

  std::printf("%d mismatches\n", bad);
  return bad ? 1 : 0;
}
