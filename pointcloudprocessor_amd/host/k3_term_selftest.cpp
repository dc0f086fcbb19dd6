// k3_term_selftest -- csrc/pcp_visit_forms.hpp compiled for the host (-ffp-contract=off, std::fma): the short distortion without the
// k3 term (distort_short<false>) against the written form under cameras that pass k3_term_droppable(), on random and on extreme
// operands, and the predicate itself on cameras that pass and that fail.  What is compared is what a visit makes of the result:
// the verdicts of the pixel rule and of the cell rule, the pixel and the cell under them, and (u, v) bit for bit wherever the
// written form accepts.  CPU only: the device runs the same text through pcp_selftest_k3_term().  Exit code 0 iff nothing disagrees.
// usage: k3_term_selftest [random samples per camera]
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
static uint64_t bits_of(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}
static bool same(double a, double b) { return (a != a && b != b) || bits_of(a) == bits_of(b); }

struct Camera {
  vf::Distortion d;
  double fx, fy, cx, cy;
  int32_t w, h, ds;
};

struct Verdict {
  bool image_ok, map_ok;
  int32_t pixel, cell;
};
// the two truncation rules as the reference writes them (PointCloudProcessor.cpp:752-754, view_culling.cpp:86-90, :116)
static Verdict verdict_of(const Camera &c, double xd, double yd, double &u, double &v) {
  u = c.fx * xd + c.cx;
  v = c.fy * yd + c.cy;
  Verdict r;
  r.image_ok = u > -1.0 && u < static_cast<double>(c.w) && v > -1.0 && v < static_cast<double>(c.h);
  r.pixel = r.image_ok ? static_cast<int32_t>(v) * c.w + static_cast<int32_t>(u) : 0;
  const float ds = static_cast<float>(c.ds);
  const int32_t cell = vf::map_cell_written(static_cast<float>(u) / ds, static_cast<float>(v) / ds, static_cast<float>(c.w),
                                            static_cast<float>(c.h), c.w / c.ds, c.h / c.ds);
  r.map_ok = cell >= 0;
  r.cell = r.map_ok ? cell : 0;
  return r;
}

static long check_forms(long samples) {
  const double inf = INFINITY, nan = NAN;
  const vf::Distortion ref = {0.003043514741045163, 0.06634739187544138, 0.0, -0.000217681797407554, -0.0006654964142658197};
  std::vector<Camera> cams = {
      {ref, 2258.5, 2258.5, 960.0, 540.0, 1920, 1080, 14},                                                   // cfg
      {ref, 4818.200388954926, 4819.10345841615, 2032.4178620390019, 1535.1895959282901, 4096, 3000, 14},  // ref
      {ref, 564.625, 564.625, 240.0, 135.0, 480, 270, 14},                                                   // tiny
      {{0.0, 0.0, 0.0, 0.0, 0.0}, 600.0, 600.0, 351.5, 202.5, 703, 405, 14},                                 // no distortion at all
      {{0.1, 0.0, 0.0, 0.0, 0.0}, 600.0, -600.0, 351.5, 202.5, 703, 405, 7},                                 // k1 leads
      {{0.0, -0.02, 0.0, 0.01, 0.0}, 600.0, 600.0, 351.5, 202.5, 703, 405, 1},                               // k2 alone
      {{-0.2, 0.05, 0.0, -0.01, -0.02}, 600.0, 600.0, -351.5, 202.5, 703, 405, 14},
      {{0x1p-60, 0.0, 0.0, 0x1p60, -0x1p60}, 0x1p-20, 0x1p40, 0x1p40, -0x1p40, 703, 405, 14},  // the edges of the range
      {{-0x1p60, 0x1p-60, 0.0, -0x1p-60, 0x1p60}, 0x1p40, -0x1p-20, 0.0, 0.0, 703, 405, 14},
      {{0x1p60, 0x1p60, 0.0, 0x1p60, 0x1p60}, 0x1p40, 0x1p40, 0x1p40, 0x1p40, 703, 405, 14},
  };
  // both signs of the zero
  const size_t base = cams.size();
  for (size_t i = 0; i < base; ++i) {
    Camera c = cams[i];
    c.d.k3 = -0.0;
    cams.push_back(c);
  }
  // what the projection can hand over: quotients of promoted floats (0, +-[2^-277, 2^277]) and non-finite values; a sweep of
  // magnitudes through the point where r6 overflows (r2 near 2^341: 2^170) and where r4 does (2^256)
  std::vector<double> edge = {0.0, -0.0, inf, -inf, nan, 1.0, -1.0, 0.5, 1.0 / 3.0, 0x1p-277, -0x1p-277, 0x1p277, -0x1p277, 3.0e38 / 0x1p-149};
  for (int e = 100; e <= 190; e += 5)
    for (double m : {1.0, -1.0, 1.7}) edge.push_back(std::ldexp(m, e));
  for (int e = 168; e <= 173; ++e)
    for (double m : {1.0, -1.0, 1.2, 1.4142135623730951, -1.9}) edge.push_back(std::ldexp(m, e));
  for (int e : {-190, -150, -100, -50, 200, 230, 255, 256, 257, 270}) edge.push_back(std::ldexp(1.0, e));
  long bad = 0, done = 0, overflowed = 0;
  for (const Camera &c : cams) {
    if (!vf::distortion_is_tame(c.d.p1, c.d.p2) || !vf::k3_term_droppable(c.d, c.fx, c.fy, c.cx, c.cy)) {
      std::printf("k3 term: a camera of the test does not qualify\n");
      return 1;
    }
    auto one = [&](double xn, double yn) {
      double xa, ya, xb, yb, ua, va, ub, vb;
      vf::distort_written(c.d, xn, yn, xa, ya);
      vf::distort_short<false>(c.d, xn, yn, xb, yb);
      const Verdict a = verdict_of(c, xa, ya, ua, va), b = verdict_of(c, xb, yb, ub, vb);
      ++done;
      const double r2 = xn * xn + yn * yn;
      const bool over = std::isinf(r2 * (r2 * r2));
      overflowed += over ? 1 : 0;
      bool ok = a.image_ok == b.image_ok && a.map_ok == b.map_ok && a.pixel == b.pixel && a.cell == b.cell;
      if (a.image_ok || a.map_ok) ok = ok && same(ua, ub) && same(va, vb);
      if (!over) ok = ok && same(xa, xb) && same(ya, yb);  // cases a and b of the proof: the same bits
      if (over) ok = ok && !a.image_ok && !a.map_ok;        // case c: the written form rejects (0 inf = NaN) ...
      if (!ok) {
        if (bad < 10)
          std::printf("k3 term: xn %a yn %a: written (%a, %a) u %a v %a, without the term (%a, %a) u %a v %a\n", xn, yn, xa, ya, ua, va, xb,
                      yb, ub, vb);
        ++bad;
      }
    };
    for (double a : edge)
      for (double b : edge) one(a, b);
    for (long i = 0; i < samples; ++i) {
      // x / z, y / z of random floats over every exponent (every fourth triple: metre-scale exponents), as the kernels form them
      const uint64_t r = mix(static_cast<uint64_t>(i) * 3u + 29u), s = mix(r);
      uint32_t bx = static_cast<uint32_t>(r), by = static_cast<uint32_t>(r >> 32), bz = static_cast<uint32_t>(s);
      if (((s >> 32) & 3u) == 0u) {
        bx = (bx & 0x807fffffu) | ((121u + (bx >> 23) % 12u) << 23);
        by = (by & 0x807fffffu) | ((121u + (by >> 23) % 12u) << 23);
        bz = (bz & 0x807fffffu) | ((121u + (bz >> 23) % 12u) << 23);
      }
      const float x = f32_of(bx), y = f32_of(by), z = std::fabs(f32_of(bz));
      if (!(z > 0.0f)) continue;
      one(static_cast<double>(x) / static_cast<double>(z), static_cast<double>(y) / static_cast<double>(z));
    }
  }
  std::printf("k3 term: %ld pairs (%ld with an overflowing r6), %ld mismatches\n", done, overflowed, bad);
  if (overflowed < 1000) {
    std::printf("k3 term: the operands hardly reach the overflow of r6\n");
    ++bad;
  }
  return bad;
}

// cameras that must keep the term
static long check_predicate() {
  const double inf = INFINITY, nan = NAN;
  const vf::Distortion ref = {0.003043514741045163, 0.06634739187544138, 0.0, -0.000217681797407554, -0.0006654964142658197};
  const Camera good = {ref, 2258.5, 2258.5, 960.0, 540.0, 1920, 1080, 14};
  std::vector<Camera> fail;
  auto with = [&](auto change) {
    Camera c = good;
    change(c);
    fail.push_back(c);
  };
  for (double k3 : {0.003, -1e-300, 4.9e-324, inf, -inf, nan}) with([&](Camera &c) { c.d.k3 = k3; });
  for (double k : {0x1p-61, -0x1p-61, 0x1p61, 4.9e-324, 1e-30, inf, -inf, nan}) {
    with([&](Camera &c) { c.d.k1 = k; });
    with([&](Camera &c) { c.d.k2 = k; });
    with([&](Camera &c) { c.d.p1 = k; });
    with([&](Camera &c) { c.d.p2 = k; });
  }
  // no leading coefficient under a tangential term: xd = xn (1 + 2 p1 yn) + p2 t2 can cancel
  with([&](Camera &c) { c.d.k1 = c.d.k2 = 0.0; });
  with([&](Camera &c) { c.d.k1 = c.d.k2 = 0.0, c.d.p2 = 0.0; });
  with([&](Camera &c) { c.d.k1 = -0.0, c.d.k2 = 0.0, c.d.p1 = 0.0; });
  for (double f : {0.0, -0.0, 0x1p-21, 0x1p41, -0x1p41, inf, nan}) {
    with([&](Camera &c) { c.fx = f; });
    with([&](Camera &c) { c.fy = f; });
  }
  for (double p : {0x1p41, -0x1p41, inf, -inf, nan}) {
    with([&](Camera &c) { c.cx = p; });
    with([&](Camera &c) { c.cy = p; });
  }
  long bad = 0;
  if (!vf::k3_term_droppable(good.d, good.fx, good.fy, good.cx, good.cy)) {
    std::printf("predicate: the default camera does not qualify\n");
    ++bad;
  }
  for (const Camera &c : fail)
    if (vf::k3_term_droppable(c.d, c.fx, c.fy, c.cx, c.cy)) {
      std::printf("predicate: k1 %a k2 %a k3 %a p1 %a p2 %a fx %a fy %a cx %a cy %a qualifies\n", c.d.k1, c.d.k2, c.d.k3, c.d.p1, c.d.p2,
                  c.fx, c.fy, c.cx, c.cy);
      ++bad;
    }
  // why the last condition is there: a camera without a leading coefficient under which the form without the term accepts a
  // lane the written form rejects (xd cancels to 0 where r6 overflows, yd = yn is a pixel row)
  {
    Camera c = good;
    c.d = {0.0, 0.0, 0.0, 0x1p-170, 0.0};
    const double xn = 0x1p171, yn = -0x1p169;  // 1 + 2 p1 yn = 0
    double xa, ya, xb, yb, ua, va, ub, vb;
    vf::distort_written(c.d, xn, yn, xa, ya);
    vf::distort_short<false>(c.d, xn, yn, xb, yb);
    const Verdict a = verdict_of(c, xa, ya, ua, va);
    (void)verdict_of(c, xb, yb, ub, vb);
    if (a.image_ok || a.map_ok || !(ua != ua) || !(xb == 0.0)) {
      std::printf("predicate: the counter-example is none: written u %a, without the term xd %a\n", ua, xb);
      ++bad;
    }
  }
  std::printf("predicate: %zu cameras that keep the term, %ld mismatches\n", fail.size(), bad);
  return bad;
}

int main(int argc, char **argv) {
  const long samples = argc > 1 ? std::atol(argv[1]) : 1000000;
  const long bad = check_forms(samples) + check_predicate();
  std::printf("k3_term_selftest: %ld mismatches\n", bad);
  return bad == 0 ? 0 : 1;
}
