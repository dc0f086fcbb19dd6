// coarse_selftest -- csrc/pcp_coarse.hpp compiled for the host (CPU only: never a GPU job; meant to be built with
// -fsanitize=address,undefined as well).  Checks the parameters' bounds, the bins on and beside every edge and at the widest
// ranges against 128-bit arithmetic, the saliency rule at equality, the two least keys and their tie rule, the correspondence
// list (ratio, lone candidate, mutual), the generator's range, each refusal of a triple and the frame of an accepted one, the
// inlier test on its boundary, the refit (a planted motion recovered, the order of the pairs not showing) and the consensus
// over planted pairs among false ones.  Prints the number of mismatches; exit code 0 iff none.
//   usage: coarse_selftest [pairs]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pcp_hip.h"
#include "../csrc/pcp_coarse.hpp"

using namespace pcp;

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

static double unit(uint64_t r) { return static_cast<double>(r >> 11) * (1.0 / 9007199254740992.0); }

static pcp_coarse_params defaults() {
  pcp_coarse_params p;
  p.support_radius = 0.2f, p.normal_radius = 0.1f, p.inlier_distance = 0.05f, p.min_side = 0.3f, p.side_tolerance = 0.05f, p.min_angle_deg = 15.0f;
  p.map_stride = p.base_stride = 4, p.min_neighbours = 20, p.min_offplane_permille = 100, p.ratio_q8 = 230, p.mutual = 1, p.hypotheses = 4096;
  p.min_inliers = 10, p.seed = 1;
  return p;
}

// x' = R x + s for the rotation by `angle` about the unit axis (ax, ay, az)
struct Motion {
  double R[9], s[3];
  void of(const float *x, float *out) const {
    for (int a = 0; a < 3; ++a) out[a] = static_cast<float>(((R[3 * a] * x[0] + R[3 * a + 1] * x[1]) + R[3 * a + 2] * x[2]) + s[a]);
  }
};
static Motion motion(double angle, double sx, double sy, double sz) {
  const double n = std::sqrt(0.3 * 0.3 + 0.5 * 0.5 + 0.8 * 0.8), h = angle * 0.5;
  const double q[4] = {std::cos(h), std::sin(h) * 0.3 / n, -std::sin(h) * 0.5 / n, std::sin(h) * 0.8 / n};
  Motion m;
  rg::rotation_of(q, m.R);
  m.s[0] = sx, m.s[1] = sy, m.s[2] = sz;
  return m;
}

int main(int argc, char **argv) {
  const int64_t count = argc > 1 ? std::strtoll(argv[1], nullptr, 10) : 400;
  uint64_t bad = 0;
  auto fail = [&](const char *what, double a, double b) {
    if (bad < 10) std::fprintf(stderr, "mismatch (%s): %.17g %.17g\n", what, a, b);
    ++bad;
  };
  cg::Rule r;
  // CG9: the bounds
  {
    pcp_coarse_params p = defaults();
    if (cg::prepare(p, &r)) fail("defaults refused", 0, 0);
    if (r.t != gn::threshold_of(0.2f) || r.edge2[0] != 0 || r.edge2[7] != ((7 * 209715) / 8) * int64_t((7 * 209715) / 8)) fail("rule", r.t, static_cast<double>(r.edge2[7]));
    auto taken = [&](const char *what, pcp_coarse_params q) {
      cg::Rule x;
      if (!cg::prepare(q, &x)) fail(what, 0, 0);
    };
    pcp_coarse_params q = p;
    q.support_radius = std::nextafter(0.02f, 0.0f), taken("support_radius low", q);
    q.support_radius = std::nextafter(0.25f, 1.0f), taken("support_radius high", q);
    q.support_radius = NAN, taken("support_radius NaN", q);
    q = p, q.normal_radius = 1.5f, taken("normal_radius", q);
    q = p, q.inlier_distance = NAN, taken("inlier_distance NaN", q);
    q = p, q.inlier_distance = 0.6f, taken("inlier_distance", q);
    q = p, q.min_side = 0.0f, taken("min_side", q);
    q = p, q.side_tolerance = -0.1f, taken("side_tolerance", q);
    q = p, q.min_angle_deg = 61.0f, taken("min_angle_deg", q);
    q = p, q.map_stride = 0, taken("map_stride", q);
    q = p, q.min_neighbours = 0, taken("min_neighbours", q);
    q = p, q.min_offplane_permille = 1001, taken("permille", q);
    q = p, q.ratio_q8 = 257, taken("ratio_q8", q);
    q = p, q.mutual = 2, taken("mutual", q);
    q = p, q.hypotheses = cg::kMaxHypotheses + 1, taken("hypotheses", q);
    q = p, q.min_inliers = 2, taken("min_inliers", q);
    q = p, q.support_radius = 0.25f, q.inlier_distance = 0.5f, q.hypotheses = cg::kMaxHypotheses;
    if (cg::prepare(q, &r)) fail("upper bounds refused", 0, 0);
    if (r.edge2[7] != int64_t(229376) * 229376 || r.tau2 != (int64_t(1) << 38)) fail("upper rule", static_cast<double>(r.edge2[7]), static_cast<double>(r.tau2));
  }
  // CG2: on and beside every edge (support 0.25: e_k = k * 2^15 quanta = k / 32 m), both signs of the height, the clamp, Q2 = 0
  {
    const int32_t N[3] = {0, 0, 2048};
    cg::Axis ax;
    cg::axis_of(r.edge2, N, ax);
    const float tiny = 1.0f / 1048576.0f;
    for (int k = 1; k < 8; ++k) {
      const float e = static_cast<float>(k) / 32.0f;
      if (cg::bin_of(ax, r.t, e, 0, 0) != 8 * k || cg::bin_of(ax, r.t, e - tiny, 0, 0) != 8 * (k - 1)) fail("radial edge", k, cg::bin_of(ax, r.t, e, 0, 0));
      if (cg::bin_of(ax, r.t, 0, 0, e) != k || cg::bin_of(ax, r.t, 0, 0, -e) != k || cg::bin_of(ax, r.t, 0, 0, e - tiny) != k - 1) fail("height edge", k, cg::bin_of(ax, r.t, 0, 0, e));
    }
    if (cg::bin_of(ax, r.t, 0.25f, 0, 0) != 56 || cg::bin_of(ax, r.t, 0, 0, -0.25f) != 7 || cg::bin_of(ax, r.t, 0, 0, 0) != 0) fail("clamp / duplicate", 0, 0);
    if (cg::bin_of(ax, r.t, std::nextafter(0.25f, 1.0f), 0, 0) != -1 || cg::bin_of(ax, r.t, NAN, 0, 0) != -1) fail("beyond the support", 0, 0);
    // the widest ranges: every component of the normal at 1, offsets on the sphere
    const int32_t W[3] = {2048, -2048, 2048};
    cg::axis_of(r.edge2, W, ax);
    for (int64_t k = 0; k < count; ++k) {
      const uint64_t s = mix(static_cast<uint64_t>(k) + 11);
      double d[3] = {unit(s) - 0.5, unit(mix(s)) - 0.5, unit(mix(mix(s))) - 0.5};
      const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), want = (k % 3 == 0) ? 0.25 : 0.25 * unit(mix(s + 5));
      const float dx = static_cast<float>(d[0] / len * want), dy = static_cast<float>(d[1] / len * want), dz = static_cast<float>(d[2] / len * want);
      const int bin = cg::bin_of(ax, r.t, dx, dy, dz);
      if (bin < 0) continue;
      if (bin > 63 || !cg::bins_hold(ax, dx, dy, dz)) fail("ranges", static_cast<double>(k), bin);
      // against 128-bit arithmetic
      const __int128 q[3] = {gn::quantise(dx), gn::quantise(dy), gn::quantise(dz)};
      const __int128 h = (q[0] - q[1] + q[2]) * 2048, N2 = 3 * 2048 * 2048, Wd = (q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) * N2 - h * h;
      int ra = 0, he = 0;
      for (int e = 1; e < 8; ++e) ra += static_cast<__int128>(r.edge2[e]) * N2 <= Wd, he += static_cast<__int128>(r.edge2[e]) * N2 <= h * h;
      if (bin != 8 * ra + he) fail("bin against 128 bits", bin, 8 * ra + he);
    }
  }
  // CG2: the validity rule at equality, the scaling
  if (!cg::descriptor_ok(10, 100, 10, 9) || cg::descriptor_ok(11, 100, 10, 9) || cg::descriptor_ok(10, 101, 10, 9) || !cg::descriptor_ok(1, 0, 1, 1) ||
      cg::descriptor_ok(1, 1, 500, 500))
    fail("descriptor_ok", 0, 0);
  if (cg::scaled(7, 7) != 65535 || cg::scaled(0, 9) != 0 || cg::scaled(1, 3) != 21845 || cg::scaled(4000000, 4194303) != static_cast<uint16_t>((4000000ull * 65535ull) / 4194303ull))
    fail("scaled", cg::scaled(1, 3), 0);
  // CG3: the two least keys in any order of arrival, ties by ordinal, the list
  {
    const uint64_t keys[5] = {(5ull << 32) | 4, (2ull << 32) | 3, (9ull << 32) | 0, (2ull << 32) | 1, (7ull << 32) | 2};
    for (int rot = 0; rot < 5; ++rot) {
      cg::Best b{cg::kNoKey, cg::kNoKey};
      for (int k = 0; k < 5; ++k) cg::offer(b, keys[(k + rot) % 5]);
      if (b.best != ((2ull << 32) | 1) || b.second != ((2ull << 32) | 3)) fail("best two", static_cast<double>(b.best), static_cast<double>(b.second));
    }
    uint16_t a[64], c[64];
    for (int k = 0; k < 64; ++k) a[k] = 65535, c[k] = 0;
    if (cg::l1_of(a, c) != 64u * 65535u || cg::l1_of(c, a) != 64u * 65535u || cg::l1_of(a, a) != 0) fail("l1", cg::l1_of(a, c), 0);
    // base 0 and base 1 both prefer map 0, which prefers base 0; base 2 has a lone candidate's key; base 3 fails the ratio at 230
    const cg::Best base[4] = {{(10ull << 32) | 0, (400ull << 32) | 1}, {(12ull << 32) | 0, (300ull << 32) | 1}, {(50ull << 32) | 1, cg::kNoKey}, {(95ull << 32) | 2, (100ull << 32) | 1}};
    const cg::Best map[3] = {{(10ull << 32) | 0, (12ull << 32) | 1}, {(50ull << 32) | 2, (300ull << 32) | 1}, {(95ull << 32) | 3, cg::kNoKey}};
    std::vector<int32_t> pairs;
    cg::Rule m = r;
    m.ratio_q8 = 230, m.mutual = 1;
    cg::correspondences(m, 4, base, map, pairs);
    if (pairs != std::vector<int32_t>{0, 0, 2, 1}) fail("correspondences mutual", static_cast<double>(pairs.size()), 0);
    m.mutual = 0;
    cg::correspondences(m, 4, base, map, pairs);
    if (pairs != std::vector<int32_t>{0, 0, 1, 0, 2, 1}) fail("correspondences", static_cast<double>(pairs.size()), 0);
    m.ratio_q8 = 256;
    cg::correspondences(m, 4, base, map, pairs);
    if (pairs.size() != 8) fail("correspondences ratio 256", static_cast<double>(pairs.size()), 0);
    m.ratio_q8 = 243;  // 95 * 256 = 24320 = 243.2 * 100: just refused, and taken at 244
    cg::correspondences(m, 4, base, map, pairs);
    if (pairs.size() != 6) fail("ratio boundary", static_cast<double>(pairs.size()), 0);
    m.ratio_q8 = 244;
    cg::correspondences(m, 4, base, map, pairs);
    if (pairs.size() != 8) fail("ratio boundary taken", static_cast<double>(pairs.size()), 0);
  }
  // CG4: the generator's range; each refusal; an accepted triple's frame
  for (uint32_t h = 0; h < 2000; ++h)
    for (uint32_t s = 0; s < 3; ++s) {
      const int64_t d = cg::draw(h * 77ull, h, s, 1 + (h % 97) * 2700);
      if (d < 0 || d >= 1 + (h % 97) * 2700 || d != cg::draw(h * 77ull, h, s, 1 + (h % 97) * 2700)) fail("draw", h, static_cast<double>(d));
    }
  {
    pcp_coarse_params p = defaults();
    cg::prepare(p, &r);
    const Motion mo = motion(0.9, 2.0, -1.0, 0.5);
    const double pivot[3] = {0.5, 0.25, -1.0};
    auto code_of = [&](const float tri[9], double scale_base, uint32_t h, cg::Hypothesis *out) {
      float cb[9], cm[9];
      for (int k = 0; k < 3; ++k) mo.of(tri + 3 * k, cm + 3 * k);
      for (int a = 0; a < 9; ++a) cb[a] = static_cast<float>(tri[a] * scale_base);
      cg::Hypothesis hy;
      cg::hypothesis(r, 3, cb, cm, pivot, h, hy);
      if (out) *out = hy;
      return hy.code;
    };
    uint32_t distinct = 0, repeat = 0;
    for (uint32_t h = 0; h < 1000; ++h) {
      const int64_t t[3] = {cg::draw(1, h, 0, 3), cg::draw(1, h, 1, 3), cg::draw(1, h, 2, 3)};
      const bool d = t[0] != t[1] && t[0] != t[2] && t[1] != t[2];
      if (d && !distinct) distinct = h + 1;
      if (!d && !repeat) repeat = h + 1;
    }
    if (!distinct || !repeat) fail("no triple found", distinct, repeat);
    const float tri[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, small[9] = {0, 0, 0, 0.25f, 0, 0, 0, 0.25f, 0}, thin[9] = {0, 0, 0, 1, 0, 0, 0.5f, 0.1f, 0};
    cg::Hypothesis hy;
    if (code_of(tri, 1.0, distinct - 1, &hy) != cg::kAccepted) fail("accepted", hy.code, 0);
    for (int k = 0; k < 3; ++k) {  // the frame takes the base triangle onto the map's
      float want[3];
      mo.of(tri + 3 * k, want);
      if (!cg::inlier_pair(hy.f, 16, tri + 3 * k, want)) fail("frame", k, 0);  // (within 4 quanta)
    }
    if (code_of(tri, 1.0, repeat - 1, nullptr) != cg::kRepeat) fail("repeat", 0, 0);
    if (code_of(small, 1.0, distinct - 1, nullptr) != cg::kShortSide) fail("short side", 0, 0);
    if (code_of(tri, 1.06, distinct - 1, nullptr) != cg::kSideMismatch) fail("side mismatch", 0, 0);
    if (code_of(thin, 1.0, distinct - 1, nullptr) != cg::kThin) fail("thin", 0, 0);
  }
  // CG5: the boundary (inlier_distance 0.05: tau2 = floor((0.05f * 2^20)^2))
  {
    const int64_t edge = static_cast<int64_t>(std::floor(std::sqrt(static_cast<double>(r.tau2))));
    const float on = static_cast<float>(edge) / 1048576.0f, over = static_cast<float>(edge + 1) / 1048576.0f;
    if (!cg::inlier_of(r.tau2, on, 0, 0) || cg::inlier_of(r.tau2, over, 0, 0) || !cg::inlier_of(r.tau2, 0, -on, 0) || cg::inlier_of(r.tau2, 0, 0, -over))
      fail("inlier boundary", on, over);
    if (cg::inlier_of(int64_t(1) << 50, 1.5f, 0, 0) || cg::inlier_of(int64_t(1) << 50, 0, NAN, 0) || cg::inlier_of(int64_t(1) << 50, 0, 0, INFINITY) ||
        !cg::inlier_of(int64_t(1) << 50, 1.0f, -1.0f, 1.0f))
      fail("inlier guard", 0, 0);
  }
  // CG6: the refit recovers a planted motion, whatever the order of the pairs; the consensus finds it among false pairs
  {
    const Motion mo = motion(1.2, 3.0, -2.0, 1.0);
    const int64_t C = count;
    std::vector<float> cb(static_cast<size_t>(3 * C)), cm(static_cast<size_t>(3 * C));
    std::vector<uint8_t> flags(static_cast<size_t>(C), 1);
    for (int64_t k = 0; k < C; ++k) {
      const uint64_t s = mix(static_cast<uint64_t>(k) + 1234);
      float *b = cb.data() + 3 * k;
      b[0] = static_cast<float>(10.0 + 2.0 * unit(s)), b[1] = static_cast<float>(-4.0 + 1.5 * unit(mix(s))), b[2] = static_cast<float>(1.0 + unit(mix(mix(s))));
      mo.of(b, cm.data() + 3 * k);
      if (k % 3 == 2) {  // a false pair, far from where the motion puts it
        cm[static_cast<size_t>(3 * k)] += 0.7f;
        flags[static_cast<size_t>(k)] = 0;
      }
    }
    const double pb[3] = {11.0, -3.25, 1.5}, pm[3] = {8.0, 1.0, 2.0};
    rg::Frame f, g;
    if (cg::refit(C, cb.data(), cm.data(), flags.data(), pb, pm, f) != 0) fail("refit range", 0, 0);
    double worst = 0.0;
    for (int a = 0; a < 9; ++a) worst = std::fmax(worst, std::fabs(f.R[a] - mo.R[a]));
    // (the sums see the points through quanta of 2^-16 m: a rotation entry may be off by one quantum over the cloud's least
    // extent, 1.5e-5 m / 1 m, however few pairs there are)
    if (!(worst < 1.5e-5)) fail("refit rotation", worst, 0);
    for (int64_t k = 0; k < C; ++k)
      if (flags[static_cast<size_t>(k)] && !cg::inlier_pair(f, 64 * 64, cb.data() + 3 * k, cm.data() + 3 * k)) fail("refit pair", static_cast<double>(k), 0);
    // the pairs in reverse order: the same bytes
    std::vector<float> rb(cb.size()), rm(cm.size());
    std::vector<uint8_t> rf(flags.size());
    for (int64_t k = 0; k < C; ++k) {
      std::memcpy(rb.data() + 3 * k, cb.data() + 3 * (C - 1 - k), 12);
      std::memcpy(rm.data() + 3 * k, cm.data() + 3 * (C - 1 - k), 12);
      rf[static_cast<size_t>(k)] = flags[static_cast<size_t>(C - 1 - k)];
    }
    cg::refit(C, rb.data(), rm.data(), rf.data(), pb, pm, g);
    if (std::memcmp(&f, &g, sizeof f) != 0) fail("refit order", 0, 0);
    float far[3] = {70000.0f, 0, 0};
    uint8_t one = 1;
    if (cg::refit(1, far, far, &one, pb, pm, g) != -1) fail("refit range taken", 0, 0);
    // consensus
    pcp_coarse_params p = defaults();
    p.hypotheses = 512, p.side_tolerance = 0.01f;
    cg::prepare(p, &r);
    int64_t report[cg::kReportWords] = {0};
    rg::Frame found;
    std::vector<uint8_t> in;
    const int rc = cg::consensus(r, C, cb.data(), cm.data(), pb, pm, [&](const rg::Frame *fr, int64_t n, int64_t *counts, uint8_t *fl) {
      for (int64_t i = 0; i < n; ++i) {
        counts[i] = 0;
        for (int64_t k = 0; k < C; ++k) {
          const bool ok = cg::inlier_pair(fr[i], r.tau2, cb.data() + 3 * k, cm.data() + 3 * k);
          counts[i] += ok;
          if (fl) fl[i * C + k] = ok;
        }
      }
      return 0;
    }, report, &found, in);
    const int64_t good = C - C / 3;
    if (rc != 0 || report[cg::kStatus] != cg::kFound || report[cg::kKept] != good || report[cg::kScored] + report[cg::kRefused] != 512 || report[cg::kKept] < report[cg::kWinner])
      fail("consensus", static_cast<double>(report[cg::kKept]), static_cast<double>(good));
    for (int64_t k = 0; k < C; ++k)
      if (in[static_cast<size_t>(k)] != flags[static_cast<size_t>(k)]) fail("consensus inliers", static_cast<double>(k), in[static_cast<size_t>(k)]);
    double M[16];
    cg::matrix_of_frame(found, M);
    rg::Transform T;
    if (!rg::from_matrix(M, pb, &T)) fail("the frame is no rigid motion", 0, 0);
    r.min_inliers = static_cast<int32_t>(good + 1);
    cg::consensus(r, C, cb.data(), cm.data(), pb, pm, [&](const rg::Frame *fr, int64_t n, int64_t *counts, uint8_t *fl) {
      for (int64_t i = 0; i < n; ++i) {
        counts[i] = 0;
        for (int64_t k = 0; k < C; ++k) {
          const bool ok = cg::inlier_pair(fr[i], r.tau2, cb.data() + 3 * k, cm.data() + 3 * k);
          counts[i] += ok;
          if (fl) fl[i * C + k] = ok;
        }
      }
      return 0;
    }, report, &found, in);
    if (report[cg::kStatus] != cg::kTooFewInliers || report[cg::kKept] != 0 || report[cg::kWinner] > good) fail("too few inliers", static_cast<double>(report[cg::kWinner]), 0);
  }
  std::printf("coarse_selftest: %lld pairs, %llu mismatches\n", static_cast<long long>(count), static_cast<unsigned long long>(bad));
  return bad == 0 ? 0 : 1;
}
