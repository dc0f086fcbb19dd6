// crack_width_selftest -- csrc/pcp_crack_width.hpp compiled for the host (CPU only: never a GPU job; meant to be built with
// -fsanitize=address,undefined as well).  Known answers of the ray stage at an identity and at a distorted camera -- a
// fronto-parallel plane z = 2 whose width must be 2 du / fx, a tilted plane against the closed form, a fold-back distortion
// that must fail the ray -- the trace and rdiv on small cases, the quantisation, and the recentred moments of random windows
// through wrapped summed-area tables against direct sums in 128-bit integers.  Prints the number of mismatches; exit code 0
// iff none.   usage: crack_width_selftest [side]   (side >= 1400, the default: the tables' prefixes must pass 2^64)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/pcp_crack_width.hpp"

using namespace pcp;

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

static double unit(uint64_t r) { return static_cast<double>(r >> 11) * (1.0 / 9007199254740992.0); }

static uint64_t bad = 0;
static void fail(const char *what, double a, double b) {
  if (bad < 10) std::fprintf(stderr, "mismatch (%s): %.17g %.17g\n", what, a, b);
  ++bad;
}
static void close_to(const char *what, double got, double want, double tol) {
  if (!(std::fabs(got - want) <= tol)) fail(what, got, want);
}

// (u, v) of the camera point (X, Y, Z) through the written projection
static void project(const cw::Intrinsics &c, const double X[3], double &u, double &v) {
  double xd, yd;
  cw::distort(c, X[0] / X[2], X[1] / X[2], xd, yd);
  u = c.fx * xd + c.cx;
  v = c.fy * yd + c.cy;
}

// two points of the plane n . (X - c) = 0 seen through camera k: the rays through their projections must meet the plane
// in the points themselves, and the width is their distance
static void plane_case(const char *what, const cw::Intrinsics &k, double n[3], const double c[3], const double A[3], const double B[3]) {
  const double nc = cw::orient(n, c);
  if (!(nc < 0.0)) fail(what, nc, 0.0);
  double ua, va, ub, vb, xa, ya, xb, yb, Xa[3], Xb[3];
  project(k, A, ua, va);
  project(k, B, ub, vb);
  if (!cw::undistort(k, ua, va, xa, ya) || !cw::undistort(k, ub, vb, xb, yb)) return fail(what, 0, 1);
  if (!cw::intersect(n, nc, xa, ya, Xa) || !cw::intersect(n, nc, xb, yb, Xb)) return fail(what, 0, 2);
  for (int a = 0; a < 3; ++a) {
    close_to(what, Xa[a], A[a], 1e-9);
    close_to(what, Xb[a], B[a], 1e-9);
  }
  const double want = std::sqrt((B[0] - A[0]) * (B[0] - A[0]) + (B[1] - A[1]) * (B[1] - A[1]) + (B[2] - A[2]) * (B[2] - A[2]));
  close_to(what, cw::width_of(Xa, Xb), want, 1e-9);
}

int main(int argc, char **argv) {
  const int32_t side = argc > 1 ? static_cast<int32_t>(std::strtol(argv[1], nullptr, 10)) : 1400;
  if (side < 8 || side > 4096) {
    std::fprintf(stderr, "side must be 8..4096\n");
    return 2;
  }
  const cw::Intrinsics identity{1000.0, 1000.0, 640.0, 360.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const cw::Intrinsics distorted{1000.0, 1010.0, 640.0, 360.0, 0.003043514741045163, 0.06634739187544138, -0.000217681797407554,
                                 -0.0006654964142658197, 0.0};
  const cw::Intrinsics fold{1000.0, 1000.0, 640.0, 360.0, -8.0, 0.0, 0.0, 0.0, 0.0};  // r (1 - 8 r^2) turns back at r = 0.2

  // ---- rdiv and the trace ----
  for (int32_t a = 1; a <= 40; ++a)
    for (int32_t m = 0; m <= 40; ++m) {
      if (cw::rdiv(a * m, a) != m) fail("rdiv(a m, a)", a, m);
      const int32_t q = cw::rdiv(m, a);  // m / a to nearest, halves up: 2aq <= 2m + a < 2a(q + 1)
      if (!(2 * a * q <= 2 * m + a && 2 * m + a < 2 * a * (q + 1))) fail("rdiv rounding", m, a);
    }
  if (cw::rdiv(1, 2) != 1 || cw::rdiv(3, 2) != 2 || cw::rdiv(1, 3) != 0 || cw::rdiv(2, 3) != 1 || cw::rdiv(0, 7) != 0) fail("rdiv ties", 0, 0);
  {
    // 9 x 7, background column x = 1 and column x = 6, foreground between: from (3, 2) with v = (2, 0)
    const int32_t w = 9, h = 7;
    auto bg = [&](int32_t x, int32_t y) {
      (void)y;
      return x <= 1 || x >= 6;
    };
    const cw::Edge n = cw::trace(bg, 3, 2, 2, 0, -1, w, h), f = cw::trace(bg, 3, 2, 2, 0, +1, w, h);
    if (!n.found || n.ex != 3 || n.ey != 4 || !f.found || f.ex != 11 || f.ey != 4) fail("trace along x", n.ex, f.ex);
    if (cw::edge_distance2(n, f) != 64) fail("w2d2", cw::edge_distance2(n, f), 64);
    // a slanted direction v = (2, 1) from (3, 3): steps (1, rdiv(k, 2)) = (4, 4), (5, 4), (6, 5)
    const cw::Edge s = cw::trace(bg, 3, 3, 2, 1, +1, w, h);
    if (!s.found || s.ex != 11 || s.ey != 9) fail("trace slanted", s.ex, s.ey);
    auto none = [](int32_t, int32_t) { return false; };
    const cw::Edge o = cw::trace(none, 3, 3, -1, 3, +1, w, h);
    if (o.found || o.ex != -1 || o.ey != -1) fail("open trace", o.found, o.ex);
    auto d2 = [&](int32_t x, int32_t y) -> uint32_t { return static_cast<uint32_t>(x == 4 ? 9 : (y == 0 ? 9 : 4)); };
    if (!cw::is_centre(d2, 4, 3, w, h) || cw::is_centre(d2, 3, 3, w, h) || !cw::is_centre(d2, 0, 0, w, h)) fail("is_centre", 0, 0);
  }

  // ---- quantisation ----
  if (cw::quantise(0.5f / 65536.0f) != 0 || cw::quantise(1.5f / 65536.0f) != 2 || cw::quantise(-2.5f / 65536.0f) != -2 ||
      cw::quantise(std::nextafter(64.0f, 0.0f)) != 4194304 || cw::quantise(-63.5f) != -4161536 || cw::quantise(-0.0f) != 0)
    fail("quantise", 0, 0);
  if (!cw::member_ok(63.9f, -63.9f, 0.0f) || cw::member_ok(64.0f, 0.0f, 0.0f) || cw::member_ok(0.0f, -64.0f, 0.0f) ||
      cw::member_ok(0.0f, 0.0f, NAN) || cw::member_ok(INFINITY, 0.0f, 0.0f))
    fail("member_ok", 0, 0);
  if (!cw::radius_ok(1) || !cw::radius_ok(181) || cw::radius_ok(0) || cw::radius_ok(182)) fail("radius_ok", 0, 0);
  if (cw::floor_div(-7, 2) != -4 || cw::floor_div(7, 2) != 3 || cw::floor_div(-8, 2) != -4 || cw::floor_div(0, 5) != 0) fail("floor_div", 0, 0);

  // ---- the ray stage: fronto-parallel plane z = 2 ----
  for (const cw::Intrinsics *k : {&identity, &distorted}) {
    double n[3] = {0.0, 0.0, 1.0};
    const double c[3] = {0.3, -0.2, 2.0};
    const double A[3] = {-0.11, 0.07, 2.0}, B[3] = {-0.10, 0.075, 2.0};
    plane_case(k == &identity ? "z = 2, identity" : "z = 2, distorted", *k, n, c, A, B);
  }
  {  // identity camera, doubled edge points 12 half-pixels apart along x: the width is 2 du / fx
    double n[3] = {0.0, 0.0, -1.0};
    const double c[3] = {0.0, 0.0, 2.0};
    const double nc = cw::orient(n, c);
    double Xa[3], Xb[3];
    if (!cw::edge_point(identity, n, nc, 1401, 801, Xa) || !cw::edge_point(identity, n, nc, 1413, 801, Xb)) fail("edge_point", 0, 0);
    close_to("2 du / fx", cw::width_of(Xa, Xb), 2.0 * 6.0 / 1000.0, 1e-12);
    close_to("pixel centre", Xa[0], 2.0 * ((1401 * 0.5 + 0.5) - 640.0) / 1000.0, 1e-12);
  }
  // ---- a tilted plane against the closed form ----
  for (const cw::Intrinsics *k : {&identity, &distorted}) {
    double n[3] = {0.48, -0.28, -0.83};
    const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (double &v : n) v /= len;
    const double c[3] = {0.1, 0.2, 3.0};
    // points of the plane: X = c + s e1 + t e2 with e1, e2 orthogonal to n
    const double e1[3] = {n[2], 0.0, -n[0]}, e2[3] = {0.0, n[2], -n[1]};
    double A[3], B[3];
    for (int a = 0; a < 3; ++a) {
      A[a] = c[a] + 0.4 * e1[a] - 0.3 * e2[a];
      B[a] = c[a] + 0.41 * e1[a] - 0.31 * e2[a];
    }
    plane_case(k == &identity ? "tilted, identity" : "tilted, distorted", *k, n, c, A, B);
  }
  {  // grazing incidence and a plane behind the camera are refused
    double X[3];
    const double graze[3] = {1.0, 0.0, 0.05};
    if (cw::intersect(graze, -1.0, 0.0, 0.0, X)) fail("grazing ray", 0, 0);
    const double front[3] = {0.0, 0.0, -1.0};
    if (cw::intersect(front, 2.0, 0.0, 0.0, X)) fail("plane behind the camera", 0, 0);
    if (!cw::intersect(front, -2.0, 0.0, 0.0, X) || X[2] != 2.0) fail("plane in front", X[2], 2.0);
  }
  {  // fold-back: beyond the turning radius the fixed point does not come back to (u, v)
    double x, y;
    if (cw::undistort(fold, 640.0 + 600.0, 360.0, x, y)) fail("fold-back must fail", x, y);
    double n[3] = {0.0, 0.0, -1.0}, X[3];
    const double c[3] = {0.0, 0.0, 2.0};
    if (cw::edge_point(fold, n, cw::orient(n, c), 2 * 1240, 2 * 360, X)) fail("fold-back edge point", 0, 0);
    if (!cw::undistort(identity, 1240.0, 360.0, x, y) || x != 0.6 || y != 0.0) fail("identity undistort", x, y);
  }

  // ---- CW5: wrapped summed-area tables and the recentring against direct 128-bit sums ----
  {
    const int32_t w = side, h = side - 7 > 0 ? side - 7 : side;
    const size_t px = static_cast<size_t>(w) * h;
    std::vector<int32_t> q(3 * px);
    std::vector<uint8_t> member(px);
    std::vector<uint64_t> sat(static_cast<size_t>(cw::kOriginPlanes) * px, 0);
    for (size_t p = 0; p < px; ++p) {
      member[p] = (mix(p) & 3) != 0;
      // positions near +-63.9 m: at the default size the sum of q^2 over the image passes 2^64 and the tables wrap
      const float x = static_cast<float>(60.0 + 3.9 * unit(mix(3 * p + 1))), y = static_cast<float>(-60.0 - 3.9 * unit(mix(3 * p + 2))),
                  z = static_cast<float>(55.0 + 8.9 * unit(mix(3 * p + 3)));
      q[3 * p] = cw::quantise(x);
      q[3 * p + 1] = cw::quantise(y);
      q[3 * p + 2] = cw::quantise(z);
      if (!member[p]) continue;
      uint64_t t[cw::kOriginPlanes];
      cw::origin_terms(q[3 * p], q[3 * p + 1], q[3 * p + 2], t);
      for (int a = 0; a < cw::kOriginPlanes; ++a) sat[a * px + p] = t[a];
    }
    unsigned __int128 true_total = 0;
    for (size_t p = 0; p < px; ++p)
      if (member[p]) true_total += static_cast<unsigned __int128>(static_cast<int64_t>(q[3 * p]) * q[3 * p]);
    for (int a = 0; a < cw::kOriginPlanes; ++a) {
      uint64_t *pa = sat.data() + a * px;
      for (int32_t y = 0; y < h; ++y) {
        uint64_t *row = pa + static_cast<size_t>(y) * w;
        for (int32_t x = 1; x < w; ++x) row[x] += row[x - 1];
        if (y > 0)
          for (int32_t x = 0; x < w; ++x) row[x] += row[x - w];
      }
    }
    if (side >= 1400 && (true_total >> 64) == 0) fail("the prefix of S2xx does not pass 2^64", static_cast<double>(true_total), 0);
    for (int64_t k = 0; k < 120; ++k) {
      const int32_t x = static_cast<int32_t>(mix(7000 + k) % static_cast<uint64_t>(w)), y = static_cast<int32_t>(mix(9000 + k) % static_cast<uint64_t>(h));
      const int32_t radius = 1 + static_cast<int32_t>(mix(11000 + k) % 181);
      int32_t x0, x1, y0, y1;
      cw::window(x, radius, w, x0, x1);
      cw::window(y, radius, h, y0, y1);
      uint64_t o[cw::kOriginPlanes];
      for (int a = 0; a < cw::kOriginPlanes; ++a) {
        const uint64_t *pa = sat.data() + a * px;
        o[a] = cw::window_sum([&](int32_t qx, int32_t qy) -> uint64_t { return pa[static_cast<size_t>(qy) * w + qx]; }, x0, x1, y0, y1);
      }
      int64_t m[cw::kMomentWords];
      cw::recentre(o, m);
      // direct: n, S1, then r, then the sums of (q - r)
      __int128 n = 0, s1[3] = {0, 0, 0};
      for (int32_t yy = y0; yy < y1; ++yy)
        for (int32_t xx = x0; xx < x1; ++xx) {
          const size_t p = static_cast<size_t>(yy) * w + xx;
          if (!member[p]) continue;
          n += 1;
          for (int a = 0; a < 3; ++a) s1[a] += q[3 * p + a];
        }
      if (static_cast<__int128>(m[0]) != n) fail("n", static_cast<double>(m[0]), static_cast<double>(n));
      if (n == 0) continue;
      __int128 r[3], d1[3] = {0, 0, 0}, d2[6] = {0, 0, 0, 0, 0, 0};
      for (int a = 0; a < 3; ++a) {
        const __int128 num = 2 * s1[a] + n, den = 2 * n;
        r[a] = num / den - ((num % den != 0 && num < 0) ? 1 : 0);
      }
      for (int32_t yy = y0; yy < y1; ++yy)
        for (int32_t xx = x0; xx < x1; ++xx) {
          const size_t p = static_cast<size_t>(yy) * w + xx;
          if (!member[p]) continue;
          const __int128 d[3] = {q[3 * p] - r[0], q[3 * p + 1] - r[1], q[3 * p + 2] - r[2]};
          for (int a = 0; a < 3; ++a) d1[a] += d[a];
          const __int128 t[6] = {d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]};
          for (int e = 0; e < 6; ++e) d2[e] += t[e];
        }
      for (int a = 0; a < 3; ++a) {
        if (static_cast<__int128>(m[1 + a]) != r[a]) fail("r", static_cast<double>(m[1 + a]), static_cast<double>(r[a]));
        if (static_cast<__int128>(m[4 + a]) != d1[a]) fail("S1'", static_cast<double>(m[4 + a]), static_cast<double>(d1[a]));
      }
      for (int e = 0; e < 6; ++e)
        if (static_cast<__int128>(m[7 + e]) != d2[e]) fail("S2'", static_cast<double>(m[7 + e]), static_cast<double>(d2[e]));
      // the covariance and the centroid are the written operations
      double C[6], c[3];
      cw::covariance(m, C);
      cw::centroid(m, c);
      const volatile double prod = static_cast<double>(m[4]) * static_cast<double>(m[5]);
      const volatile double quo = prod / static_cast<double>(m[0]);
      if (C[1] != static_cast<double>(m[8]) - quo) fail("covariance", C[1], 0);
      close_to("centroid", c[0], static_cast<double>(s1[0]) / static_cast<double>(n) / 65536.0, 1e-9);
    }
  }
  std::printf("%llu mismatches\n", static_cast<unsigned long long>(bad));
  return bad ? 1 : 0;
}
