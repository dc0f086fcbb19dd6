// crack_length_selftest -- csrc/pcp_crack_length.hpp compiled for the host (CPU only: never a GPU job; meant to be built with
// -fsanitize=address,undefined as well).  Known answers of the link weight (the integer root at 0, 1, 3, 4, around perfect
// squares and at 2^40, the clamp to 1), of the tie rules of the ends and of the predecessor, and of the whole stage on a
// 200-point chain in shuffled and in descending order, a ring with two routes of equal length, a chain with every point
// doubled, and a one-point crack beside a point that is no crack point.  Prints the number of mismatches; exit code 0 iff
// none.   usage: crack_length_selftest
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../csrc/pcp_crack_length.hpp"

using namespace pcp;

static uint64_t bad = 0;
static void expect(const char *what, uint64_t got, uint64_t want) {
  if (got == want) return;
  if (bad < 10) std::fprintf(stderr, "mismatch (%s): %llu, expected %llu\n", what, (unsigned long long)got, (unsigned long long)want);
  ++bad;
}

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

constexpr float kRadius = 0.005f;

static void weight_cases() {
  expect("isqrt(0)", cl::isqrt(0), 0);
  expect("w(k = 0): the clamp", cl::weight_of_k(0), 1);
  expect("w(k = 1)", cl::weight_of_k(1), 1);
  expect("w(k = 3)", cl::weight_of_k(3), 1);
  expect("w(k = 4)", cl::weight_of_k(4), 2);
  expect("w(k = 8)", cl::weight_of_k(8), 2);
  expect("w(k = 9)", cl::weight_of_k(9), 3);
  for (uint64_t s : {2ull, 3ull, 1000ull, 4096ull, 65535ull, 65536ull, 724077ull, 1048575ull, 1048576ull}) {
    expect("w(s^2 - 1)", cl::weight_of_k(s * s - 1), s - 1);
    expect("w(s^2)", cl::weight_of_k(s * s), s);
    if (s * s + 1 <= (1ull << 40)) expect("w(s^2 + 1)", cl::weight_of_k(s * s + 1), s);
  }
  expect("w(k = 2^40)", cl::weight_of_k(1ull << 40), 1ull << 20);
  expect("w(k = 2^40 - 1)", cl::weight_of_k((1ull << 40) - 1), (1ull << 20) - 1);
  for (uint64_t i = 0; i < 200000; ++i) {  // the definition, on pseudo-random k <= 2^40
    const uint64_t k = mix(i) % ((1ull << 40) + 1), w = cl::isqrt(k);
    if (!(w * w <= k && k < (w + 1) * (w + 1))) expect("isqrt: w^2 <= k < (w + 1)^2", 0, 1);
  }
  expect("w(d2 = 0): the clamp", cl::weight(0.0f), 1);
  expect("w(d2 = 2^-40)", cl::weight(std::ldexp(1.0f, -40)), 1);
  expect("w(d2 = 2^-41): the clamp", cl::weight(std::ldexp(1.0f, -41)), 1);
  expect("w(d2 = 2^-38)", cl::weight(std::ldexp(1.0f, -38)), 2);
  expect("w(d2 = 1)", cl::weight(1.0f), 1048576);
  expect("w(d2 = 0.25)", cl::weight(0.25f), 524288);
  expect("w(d2 = 2^-16)", cl::weight(std::ldexp(1.0f, -16)), 4096);
  expect("w(d2 = 2.5e-5)", cl::weight(2.5e-5f), 5242);  // sqrt(2.5e-5) * 2^20 = 5242.87...
  expect("w(denormal)", cl::weight(std::ldexp(1.0f, -140)), 1);
}

static void tie_cases() {
  expect("end: larger D", cl::end_better(5, 9, 4, 1), 1);
  expect("end: smaller D", cl::end_better(4, 1, 5, 9), 0);
  expect("end: equal D, lower index", cl::end_better(5, 2, 5, 3), 1);
  expect("end: equal D, higher index", cl::end_better(5, 3, 5, 2), 0);
  expect("end: itself", cl::end_better(5, 3, 5, 3), 0);
  expect("pred: D_j + w = D_i", cl::pred_ok(10, 5, 15), 1);
  expect("pred: D_j + w > D_i", cl::pred_ok(11, 5, 15), 0);
  expect("pred: D_j + w < D_i", cl::pred_ok(9, 5, 15), 0);
  expect("pred: not reached", cl::pred_ok(cl::kNoPos, 1, 0), 0);  // (2^64 - 1 + 1 wraps to 0)
  expect("pred: first candidate", cl::pred_better(7, -1), 1);
  expect("pred: lower index", cl::pred_better(3, 7), 1);
  expect("pred: higher index", cl::pred_better(7, 3), 0);
}

static cl::HostResult run(const std::vector<float> &xyz, const std::vector<uint32_t> &views, const std::vector<uint64_t> *sum_q = nullptr) {
  cl::HostResult res;
  cl::lengths_brute(static_cast<int64_t>(views.size()), xyz.data(), views.data(), sum_q ? sum_q->data() : nullptr, 1,
                    gn::threshold_of(kRadius), res);
  return res;
}

// a straight chain spaced 0.9 r: place p of the chain is point order[p]
static void chain_case(const char *what, const std::vector<int32_t> &order) {
  const size_t n = order.size();
  std::vector<float> xyz(3 * n, 0.0f), at(n);
  for (size_t p = 0; p < n; ++p) at[p] = static_cast<float>(0.9 * kRadius * static_cast<double>(p));
  for (size_t p = 0; p < n; ++p) xyz[3 * static_cast<size_t>(order[p])] = at[p];
  std::vector<uint32_t> views(n, 1);
  std::vector<uint64_t> sum_q(n);
  for (size_t i = 0; i < n; ++i) sum_q[i] = 100 + i;  // one view each: w = sum_q
  const cl::HostResult res = run(xyz, views, &sum_q);
  std::vector<uint64_t> along(n, 0);  // only neighbours in the chain are linked: the distance from place 0
  for (size_t p = 1; p < n; ++p) along[p] = along[p - 1] + cl::weight(cl::d2_of(at[p] - at[p - 1], 0.0f, 0.0f));
  expect(what, res.ids.size(), 1);
  if (res.ids.size() != 1) return;
  expect(what, static_cast<uint64_t>(res.ids[0]), 0);
  // s0 = point 0 lies at place q; a is the extreme farther from it (the lower index on a tie), b the other one
  size_t q = 0;
  while (order[q] != 0) ++q;
  const uint64_t to_first = along[q], to_last = along[n - 1] - along[q];
  const bool a_is_last = cl::end_better(to_last, order[n - 1], to_first, order[0]);
  const int32_t a = a_is_last ? order[n - 1] : order[0], b = a_is_last ? order[0] : order[n - 1];
  expect(what, static_cast<uint64_t>(res.rows[0]), static_cast<uint64_t>(a));
  expect(what, static_cast<uint64_t>(res.rows[1]), static_cast<uint64_t>(b));
  expect(what, static_cast<uint64_t>(res.rows[2]), along[n - 1]);
  expect(what, static_cast<uint64_t>(res.rows[3]), n - 1);
  expect(what, static_cast<uint64_t>(res.rows[4]), 100 * n + n * (n - 1) / 2);
  expect(what, static_cast<uint64_t>(res.rows[5]), 100);
  expect(what, static_cast<uint64_t>(res.rows[6]), 100 + n - 1);
  expect(what, res.path.size(), n);
  expect(what, static_cast<uint64_t>(res.offsets[1]), n);
  for (size_t p = 0; p < n && res.path.size() == n; ++p) {
    const size_t place = a_is_last ? n - 1 - p : p;
    expect(what, static_cast<uint64_t>(res.path[p]), static_cast<uint64_t>(order[place]));
    expect(what, res.pos[static_cast<size_t>(order[place])], a_is_last ? along[n - 1] - along[place] : along[place]);
  }
}

// a square loop on the lattice of spacing 2^-8 m: every link has d2 = 2^-16 exactly (the diagonal and two steps are beyond
// 5 mm), so every weight is 4096 and the two routes between opposite points are equal to the unit
static void ring_case() {
  const int side = 26, P = 4 * (side - 1);  // 100 points, numbered around the loop
  const float h = 1.0f / 256.0f;
  std::vector<float> xyz;
  for (int k = 0; k < P; ++k) {
    const int e = k / (side - 1), o = k % (side - 1);
    const int x = e == 0 ? o : e == 1 ? side - 1 : e == 2 ? side - 1 - o : 0;
    const int y = e == 0 ? 0 : e == 1 ? o : e == 2 ? side - 1 : side - 1 - o;
    xyz.push_back(static_cast<float>(x) * h);
    xyz.push_back(static_cast<float>(y) * h);
    xyz.push_back(0.25f);
  }
  const cl::HostResult res = run(xyz, std::vector<uint32_t>(static_cast<size_t>(P), 1));
  expect("ring: one crack", res.ids.size(), 1);
  if (res.ids.size() != 1) return;
  expect("ring: a = the point opposite the label", static_cast<uint64_t>(res.rows[0]), P / 2);
  expect("ring: b = the label", static_cast<uint64_t>(res.rows[1]), 0);
  expect("ring: length", static_cast<uint64_t>(res.rows[2]), 4096ull * (P / 2));
  expect("ring: hops", static_cast<uint64_t>(res.rows[3]), P / 2);
  expect("ring: entries", res.path.size(), P / 2 + 1);
  // from b both neighbours 1 and P - 1 are predecessors: the lower index wins, and the path runs a = P/2, P/2 - 1, ..., 1, 0
  for (size_t p = 0; p < res.path.size(); ++p) expect("ring: the tie goes to the lower index", static_cast<uint64_t>(res.path[p]), P / 2 - p);
  for (int k = 0; k < P; ++k) expect("ring: pos", res.pos[static_cast<size_t>(k)], 4096ull * static_cast<uint64_t>(std::abs(k - P / 2)));
}

// the ascending chain with every point twice (point n + p = point p): a double weighs 1, the lower indices win every tie
static void duplicates_case() {
  const size_t n = 60;
  std::vector<float> xyz(6 * n, 0.0f);
  for (size_t p = 0; p < n; ++p) xyz[3 * p + 1] = xyz[3 * (n + p) + 1] = static_cast<float>(0.9 * kRadius * static_cast<double>(p));
  const cl::HostResult res = run(xyz, std::vector<uint32_t>(2 * n, 1));
  std::vector<uint64_t> along(n, 0);
  for (size_t p = 1; p < n; ++p) along[p] = along[p - 1] + cl::weight(cl::d2_of(0.0f, xyz[3 * p + 1] - xyz[3 * (p - 1) + 1], 0.0f));
  expect("duplicates: one crack", res.ids.size(), 1);
  if (res.ids.size() != 1) return;
  expect("duplicates: a", static_cast<uint64_t>(res.rows[0]), n - 1);
  expect("duplicates: b", static_cast<uint64_t>(res.rows[1]), 0);
  expect("duplicates: length", static_cast<uint64_t>(res.rows[2]), along[n - 1]);
  expect("duplicates: hops", static_cast<uint64_t>(res.rows[3]), n - 1);
  expect("duplicates: entries", res.path.size(), n);
  for (size_t p = 0; p < res.path.size(); ++p) expect("duplicates: path", static_cast<uint64_t>(res.path[p]), n - 1 - p);
  for (size_t p = 0; p < n; ++p) {
    expect("duplicates: pos", res.pos[p], along[n - 1] - along[p]);
    expect("duplicates: pos of the double", res.pos[n + p], p == n - 1 ? 1 : along[n - 1] - along[p]);
  }
}

static void single_case() {
  const std::vector<float> xyz = {9.0f, 9.0f, 9.0f, 1.0f, 2.0f, 3.0f, 1.001f, 2.0f, 3.0f};
  const std::vector<uint32_t> views = {0, 1, 0};
  const std::vector<uint64_t> sum_q = {0, 777, 0};
  const cl::HostResult res = run(xyz, views, &sum_q);
  expect("single: one crack", res.ids.size(), 1);
  if (res.ids.size() != 1) return;
  expect("single: id", static_cast<uint64_t>(res.ids[0]), 1);
  const int64_t want[7] = {1, 1, 0, 0, 777, 777, 777};
  for (int k = 0; k < 7; ++k) expect("single: row", static_cast<uint64_t>(res.rows[static_cast<size_t>(k)]), static_cast<uint64_t>(want[k]));
  expect("single: entries", res.path.size(), 1);
  expect("single: path", static_cast<uint64_t>(res.path[0]), 1);
  expect("single: pos", res.pos[1], 0);
  expect("single: no crack point", res.pos[0], cl::kNoPos);
  expect("single: no crack point", res.pos[2], cl::kNoPos);
  const cl::HostResult none = run({}, {});
  expect("empty: rows", none.ids.size(), 0);
  expect("empty: offsets", none.offsets.size(), 1);
}

int main() {
  weight_cases();
  tie_cases();
  const size_t n = 200;
  std::vector<int32_t> order(n);
  std::iota(order.begin(), order.end(), 0);
  for (size_t i = n - 1; i > 0; --i) std::swap(order[i], order[static_cast<size_t>(mix(i) % (i + 1))]);
  chain_case("chain, shuffled", order);
  for (size_t p = 0; p < n; ++p) order[p] = static_cast<int32_t>(n - 1 - p);
  chain_case("chain, descending", order);
  ring_case();
  duplicates_case();
  single_case();
  std::printf("crack_length_selftest: %llu mismatches\n", (unsigned long long)bad);
  return bad ? 1 : 0;
}
