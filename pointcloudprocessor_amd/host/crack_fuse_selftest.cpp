// crack_fuse_selftest -- csrc/pcp_crack_fuse.hpp compiled for the host (CPU only: never a GPU job; meant to be built with
// -fsanitize=address,undefined as well).  Known answers of the width quantum (ties to even, the clamp), the state update
// applied in two orders, the rounding of the fused results, the link test at the threshold and at the next float above it,
// the ordered-integer form of a coordinate, and the brute-force labelling of a chain, a ring and two clusters.  Prints the
// number of mismatches; exit code 0 iff none.   usage: crack_fuse_selftest
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/pcp_crack_fuse.hpp"

using namespace pcp;

static uint64_t bad = 0;
static void expect(const char *what, uint64_t got, uint64_t want) {
  if (got == want) return;
  if (bad < 10) std::fprintf(stderr, "mismatch (%s): %llu, expected %llu\n", what, (unsigned long long)got, (unsigned long long)want);
  ++bad;
}

static uint32_t bits_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

static void quantum_cases() {
  const float q = 1.0f / 1048576.0f;  // one quantum
  expect("q(0)", cf::quantum(0.0f), 0);
  expect("q(1 quantum)", cf::quantum(q), 1);
  expect("q(0.5 quanta): tie to even", cf::quantum(0.5f * q), 0);
  expect("q(1.5 quanta): tie to even", cf::quantum(1.5f * q), 2);
  expect("q(2.5 quanta): tie to even", cf::quantum(2.5f * q), 2);
  expect("q(0.75 quanta)", cf::quantum(0.75f * q), 1);
  expect("q(3 mm)", cf::quantum(0.003f), 3146);  // 0.003f * 2^20 = 3145.728...
  expect("q(1 m)", cf::quantum(1.0f), 1048576);
  const float below = std::nextafterf(2048.0f, 0.0f);  // 2047.9998779296875 = 2048 - 2^-13: (2^31 - 2^7) quanta exactly
  expect("q(just below 2048)", cf::quantum(below), 2147483520u);
  expect("q(2048): the clamp", cf::quantum(2048.0f), 0x7fffffffu);
  expect("q(1e9): the clamp", cf::quantum(1e9f), 0x7fffffffu);
  expect("q(inf): the clamp", cf::quantum(INFINITY), 0x7fffffffu);
  expect("q(nan): the clamp", cf::quantum(NAN), 0x7fffffffu);
}

struct View {
  uint8_t flag;
  float width, range;
  int32_t frame;
};

static void apply(cf::State &s, const View &v) { cf::update(s, v.flag, v.width, bits_of(v.range), v.frame); }

static void state_cases() {
  cf::State e;
  cf::clear(e);
  expect("clear: seen", e.seen, 0);
  expect("clear: min_q", e.min_q, 0xffffffffu);
  expect("clear: best_key", e.best_key, ~0ull);
  expect("w of no view", cf::fused_w(e.sum_q, e.views), 0);
  expect("best_frame of no view", static_cast<uint32_t>(cf::best_frame(e.best_key, e.views)), 0xffffffffu);
  expect("width_mean of no view", bits_of(cf::width_mean(e.sum_q, e.views)), 0);
  // six keyframes: two without WIDTH, one with CENTRE, two at the same range (the lower keyframe wins)
  const View views[6] = {{64, 0.004f, 3.0f, 5},      {1, 0.0f, 1.0f, 1},       {64 | 2, 0.002f, 2.5f, 4},
                         {64, 0.003f, 2.5f, 2},      {1 | 4 | 8, 0.0f, 0.5f, 0}, {64, 0.001f, 7.0f, 3}};
  cf::State a, b;
  cf::clear(a);
  cf::clear(b);
  for (int k = 0; k < 6; ++k) apply(a, views[k]);
  const int other[6] = {3, 5, 0, 4, 2, 1};
  for (int k = 0; k < 6; ++k) apply(b, views[other[k]]);
  expect("two orders: seen", a.seen, b.seen);
  expect("two orders: views", a.views, b.views);
  expect("two orders: centres", a.centres, b.centres);
  expect("two orders: sum_q", a.sum_q, b.sum_q);
  expect("two orders: min_q", a.min_q, b.min_q);
  expect("two orders: max_q", a.max_q, b.max_q);
  expect("two orders: best_key", a.best_key, b.best_key);
  expect("two orders: best_q", a.best_q, b.best_q);
  expect("seen", a.seen, 6);
  expect("views", a.views, 4);
  expect("centres", a.centres, 1);
  const uint32_t q4 = cf::quantum(0.004f), q2 = cf::quantum(0.002f), q3 = cf::quantum(0.003f), q1 = cf::quantum(0.001f);
  expect("sum_q", a.sum_q, static_cast<uint64_t>(q4) + q2 + q3 + q1);
  expect("min_q", a.min_q, q1);
  expect("max_q", a.max_q, q4);
  expect("best_frame: the equal range goes to the lower keyframe", static_cast<uint32_t>(cf::best_frame(a.best_key, a.views)), 2);
  expect("best_q", a.best_q, q3);
  expect("best_key", a.best_key, (static_cast<uint64_t>(bits_of(2.5f)) << 32) | 2u);
}

static void result_cases() {
  // CF5: floor((2 sum + views) / (2 views)) = the mean rounded to nearest, halves up
  expect("w(10, 4) = 2.5 -> 3", cf::fused_w(10, 4), 3);
  expect("w(9, 4) = 2.25 -> 2", cf::fused_w(9, 4), 2);
  expect("w(11, 4) = 2.75 -> 3", cf::fused_w(11, 4), 3);
  expect("w(7, 2) = 3.5 -> 4", cf::fused_w(7, 2), 4);
  expect("w(5, 1)", cf::fused_w(5, 1), 5);
  expect("w at the clamp", cf::fused_w(4096ull * 0x7fffffffull, 4096), 0x7fffffffu);
  expect("width_mean(3 quanta / 2)", bits_of(cf::width_mean(3, 2)), bits_of(1.5f / 1048576.0f));
  expect("width_mean(1048576, 1) = 1 m", bits_of(cf::width_mean(1048576, 1)), bits_of(1.0f));
  // (double)(1 / 3) * 2^-20 rounded to fp32 once
  expect("width_mean(1, 3)", bits_of(cf::width_mean(1, 3)), bits_of(static_cast<float>((1.0 / 3.0) * (1.0 / 1048576.0))));
  expect("width_best(3146)", bits_of(cf::width_best(3146, 1)), bits_of(static_cast<float>(3146.0 / 1048576.0)));
  expect("width_best without a view", bits_of(cf::width_best(3146, 0)), 0);
}

static void link_cases() {
  const float r = 0.02f, t = gn::threshold_of(r), above = std::nextafterf(t, 1.0f);
  if (!(static_cast<double>(t) <= static_cast<double>(r) * r) || static_cast<double>(above) <= static_cast<double>(r) * r) {
    std::fprintf(stderr, "mismatch (threshold_of)\n");
    ++bad;
  }
  // offsets along one axis whose square is exactly t / just above it cannot be written in general; test the predicate on d2
  // through axis-aligned offsets d with d * d rounded: search the float d with fl(d * d) == t
  float d = std::sqrt(t);
  while (d * d > t) d = std::nextafterf(d, 0.0f);
  while (std::nextafterf(d, 1.0f) * std::nextafterf(d, 1.0f) <= t) d = std::nextafterf(d, 1.0f);
  const float d_up = std::nextafterf(d, 1.0f);
  expect("link at the largest offset with d*d <= t", cf::linked(d, 0.0f, 0.0f, t), 1);
  expect("link: symmetric", cf::linked(-d, 0.0f, 0.0f, t), 1);
  expect("no link one float further", cf::linked(d_up, 0.0f, 0.0f, t), 0);
  expect("link on another axis", cf::linked(0.0f, 0.0f, d, t), 1);
  expect("link of a point with its duplicate", cf::linked(0.0f, 0.0f, 0.0f, t), 1);
  expect("no link through a NaN", cf::linked(NAN, 0.0f, 0.0f, t), 0);
  // the association (dx*dx + dy*dy) + dz*dz
  const float dx = 0.011f, dy = 0.012f, dz = 0.0115f;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  expect("link at d2 == threshold", cf::linked(dx, dy, dz, d2), 1);
  expect("no link with the threshold one float below d2", cf::linked(dx, dy, dz, std::nextafterf(d2, 0.0f)), 0);
  // the ordered integers
  const float vals[8] = {-INFINITY, -3.5f, -1e-30f, -0.0f, 0.0f, 1e-30f, 2.0f, INFINITY};
  for (int k = 0; k + 1 < 8; ++k) expect("order_bits ascends", cf::order_bits(vals[k]) < cf::order_bits(vals[k + 1]), 1);
  for (int k = 0; k < 8; ++k) expect("value_of inverts order_bits", bits_of(cf::value_of(cf::order_bits(vals[k]))), bits_of(vals[k]));
  cf::Box b;
  cf::clear(b);
  cf::add(b, 1.0f, -2.0f, 0.5f);
  cf::add(b, -1.0f, 3.0f, 0.5f);
  expect("box min x", bits_of(cf::value_of(b.lo[0])), bits_of(-1.0f));
  expect("box max y", bits_of(cf::value_of(b.hi[1])), bits_of(3.0f));
  expect("box min z = max z", b.lo[2], b.hi[2]);
}

// labels against what the construction says: `want[i]` = the expected label
static void label_case(const char *what, const std::vector<float> &xyz, const std::vector<uint32_t> &views, int32_t min_views, float radius,
                       const std::vector<int32_t> &want, int64_t want_components) {
  const int64_t n = static_cast<int64_t>(views.size());
  std::vector<int32_t> label(static_cast<size_t>(n) + 1, 12345);
  const int64_t got = cf::label_brute(n, xyz.data(), views.data(), min_views, gn::threshold_of(radius), label.data());
  expect(what, static_cast<uint64_t>(got), static_cast<uint64_t>(want_components));
  for (int64_t i = 0; i < n; ++i) expect(what, static_cast<uint32_t>(label[static_cast<size_t>(i)]), static_cast<uint32_t>(want[static_cast<size_t>(i)]));
  expect("the labels end where they should", static_cast<uint32_t>(label[static_cast<size_t>(n)]), 12345);
}

static void label_cases() {
  const float r = 0.02f;
  const int n = 200;
  {  // a chain in a shuffled order: place p of the chain is point perm[p]; one component, labelled 0
    std::vector<int> perm(n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(perm[i], perm[static_cast<int>(mix(i) % static_cast<uint64_t>(i + 1))]);
    std::vector<float> xyz(3 * n, 0.0f);
    for (int p = 0; p < n; ++p) xyz[3 * perm[p]] = 0.9f * r * static_cast<float>(p);
    label_case("chain", xyz, std::vector<uint32_t>(n, 1), 1, r, std::vector<int32_t>(n, 0), 1);
    // the same chain cut in the middle: the point at place 100 has too few views
    std::vector<uint32_t> views(n, 3);
    views[perm[100]] = 2;
    std::vector<int32_t> want(n);
    int lo_a = n, lo_b = n;
    for (int p = 0; p < 100; ++p) lo_a = std::min(lo_a, perm[p]);
    for (int p = 101; p < n; ++p) lo_b = std::min(lo_b, perm[p]);
    for (int p = 0; p < n; ++p) want[perm[p]] = p < 100 ? lo_a : (p == 100 ? -1 : lo_b);
    label_case("cut chain", xyz, views, 3, r, want, 2);
    // a descending chain: every union hangs the previous root under a new one
    for (int p = 0; p < n; ++p) xyz[3 * (n - 1 - p)] = 0.9f * r * static_cast<float>(p);
    label_case("descending chain", xyz, std::vector<uint32_t>(n, 1), 1, r, std::vector<int32_t>(n, 0), 1);
  }
  {  // a ring of 200 points with chord 0.8 r, one non-finite point among them
    std::vector<float> xyz(3 * (n + 1), 0.0f);
    const double rad = 0.8 * r / (2.0 * std::sin(M_PI / n));
    for (int i = 0; i < n; ++i) {
      xyz[3 * i] = static_cast<float>(rad * std::cos(2.0 * M_PI * i / n));
      xyz[3 * i + 1] = static_cast<float>(rad * std::sin(2.0 * M_PI * i / n));
    }
    xyz[3 * n + 2] = NAN;
    std::vector<int32_t> want(n + 1, 0);
    want[n] = -1;
    label_case("ring", xyz, std::vector<uint32_t>(n + 1, 1), 1, r, want, 1);
  }
  {  // two clusters of 100 points inside balls of 0.3 r, 5 r apart, interleaved in the input: labels 0 and 1
    std::vector<float> xyz(3 * n);
    std::vector<int32_t> want(n);
    for (int i = 0; i < n; ++i) {
      for (int a = 0; a < 3; ++a) xyz[3 * i + a] = 0.3f * r * (static_cast<float>(mix(7 * i + a) % 1000) / 1000.0f - 0.5f);
      if (i & 1) xyz[3 * i] += 5.0f * r;
      want[i] = i & 1;
    }
    label_case("two clusters", xyz, std::vector<uint32_t>(n, 1), 1, r, want, 2);
    label_case("no crack point", xyz, std::vector<uint32_t>(n, 0), 1, r, std::vector<int32_t>(n, -1), 0);
  }
}

int main() {
  quantum_cases();
  state_cases();
  result_cases();
  link_cases();
  label_cases();
  std::printf("crack_fuse_selftest: %llu mismatches\n", (unsigned long long)bad);
  return bad == 0 ? 0 : 1;
}
