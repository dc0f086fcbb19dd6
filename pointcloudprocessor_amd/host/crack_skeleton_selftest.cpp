// crack_skeleton_selftest -- csrc/pcp_crack_skeleton.hpp compiled for the host (CPU only: never a GPU job; meant to be built
// with -fsanitize=address,undefined as well).  Known answers of CS2 at its boundary (step_q = w_max is taken, w_max - 1 is
// not), of the band at pos = 0, step_q - 1 and step_q, of the quantum of negative and sub-quantum coordinates, and of the
// whole stage on a 200-point chain in shuffled order (as many nodes as bands, two ends), the lattice square ring of the
// length self-test (one loop, no end), and a one-point crack beside points that are no crack points.  Prints the number of
// mismatches; exit code 0 iff none.   usage: crack_skeleton_selftest
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <vector>

#include "../csrc/pcp_crack_skeleton.hpp"

using namespace pcp;

static uint64_t bad = 0;
static void expect(const char *what, int64_t got, int64_t want) {
  if (got == want) return;
  if (bad < 10) std::fprintf(stderr, "mismatch (%s): %lld, expected %lld\n", what, (long long)got, (long long)want);
  ++bad;
}

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

constexpr float kRadius = 0.005f;

static void step_cases() {
  const float t = gn::threshold_of(kRadius);
  const uint64_t wm = cs::w_max_of(t);
  expect("w_max(5 mm)", static_cast<int64_t>(wm), 5242);
  expect("w_max is the weight at the threshold", static_cast<int64_t>(wm), static_cast<int64_t>(cl::weight(t)));
  expect("step_q = w_max", cs::step_q_ok(wm, t), 1);
  expect("step_q = w_max - 1", cs::step_q_ok(wm - 1, t), 0);
  const float at = static_cast<float>(wm) / 1048576.0f, below = static_cast<float>(wm - 1) / 1048576.0f;  // (exact)
  expect("step_q of w_max * 2^-20", static_cast<int64_t>(cs::step_q_of(at)), static_cast<int64_t>(wm));
  expect("step = w_max * 2^-20", cs::step_ok(at, t), 1);
  expect("step = (w_max - 1) * 2^-20", cs::step_ok(below, t), 0);
  expect("step just below w_max * 2^-20 truncates to w_max - 1", cs::step_ok(std::nextafter(at, 0.0f), t), 0);
  expect("step = 16", cs::step_ok(16.0f, t), 1);
  expect("step above 16", cs::step_ok(std::nextafter(16.0f, 17.0f), t), 0);
  expect("step = 0", cs::step_ok(0.0f, t), 0);
  expect("step < 0", cs::step_ok(-0.01f, t), 0);
  expect("step = NaN", cs::step_ok(std::numeric_limits<float>::quiet_NaN(), t), 0);
  expect("step = inf", cs::step_ok(std::numeric_limits<float>::infinity(), t), 0);
  expect("step_q(0.01)", static_cast<int64_t>(cs::step_q_of(0.01f)), 10485);  // 0.01f * 2^20 = 10485.76
  expect("step_q(16)", static_cast<int64_t>(cs::step_q_of(16.0f)), 1 << 24);
  expect("w_max(1 m)", static_cast<int64_t>(cs::w_max_of(gn::threshold_of(1.0f))), 1 << 20);
  const uint64_t s = cs::step_q_of(0.01f);
  expect("band(0)", static_cast<int64_t>(cs::band(0, s)), 0);
  expect("band(step_q - 1)", static_cast<int64_t>(cs::band(s - 1, s)), 0);
  expect("band(step_q)", static_cast<int64_t>(cs::band(s, s)), 1);
  expect("band(2 step_q - 1)", static_cast<int64_t>(cs::band(2 * s - 1, s)), 1);
}

static void quant_cases() {
  expect("q(0)", cs::quant(0.0f), 0);
  expect("q(-0)", cs::quant(-0.0f), 0);
  expect("q(2^-20)", cs::quant(std::ldexp(1.0f, -20)), 1);
  expect("q(2^-21): below the quantum", cs::quant(std::ldexp(1.0f, -21)), 0);
  expect("q(-2^-21): the floor", cs::quant(-std::ldexp(1.0f, -21)), -1);
  expect("q(-2^-20)", cs::quant(-std::ldexp(1.0f, -20)), -1);
  expect("q(-(2^-20 + 2^-40))", cs::quant(-(std::ldexp(1.0f, -20) + std::ldexp(1.0f, -40))), -2);
  expect("q(denormal)", cs::quant(std::ldexp(1.0f, -140)), 0);
  expect("q(-denormal)", cs::quant(-std::ldexp(1.0f, -140)), -1);
  expect("q(1.5)", cs::quant(1.5f), 1572864);
  expect("q(-1.5)", cs::quant(-1.5f), -1572864);
  expect("q(2^20)", cs::quant(1048576.0f), int64_t(1) << 40);
  expect("q(-2^20)", cs::quant(-1048576.0f), -(int64_t(1) << 40));
  expect("coordinate 2^20", cs::coord_ok(1048576.0f), 1);
  expect("coordinate -2^20", cs::coord_ok(-1048576.0f), 1);
  expect("coordinate above 2^20", cs::coord_ok(std::nextafter(1048576.0f, 2e6f)), 0);
  expect("coordinate NaN", cs::coord_ok(std::numeric_limits<float>::quiet_NaN()), 0);
  expect("sums of 65536 points at 2^20 m", cs::sums_fit(65536, 1048576.0f), 1);
  expect("sums of 2^31 points at 2^20 m", cs::sums_fit(int64_t(1) << 31, 1048576.0f), 0);
  expect("edge key orders as the pair", cs::edge_key(1, 0) > cs::edge_key(0, 0x7fffffff), 1);
  expect("edge key: u", cs::key_u(cs::edge_key(123456, 7)), 123456);
  expect("edge key: v", cs::key_v(cs::edge_key(123456, 0x7fffffff)), 0x7fffffff);
}

static cs::HostResult run(const std::vector<float> &xyz, const std::vector<uint32_t> &views, uint64_t step_q,
                          const std::vector<uint64_t> *sum_q = nullptr) {
  cs::HostResult res;
  const cs::Brute how = cs::skeleton_brute(static_cast<int64_t>(views.size()), xyz.data(), views.data(), sum_q ? sum_q->data() : nullptr, 1,
                                           gn::threshold_of(kRadius), step_q, res);
  expect("the stage runs", how, cs::kBruteOk);
  return res;
}

// a straight chain spaced 0.9 r along -x, shuffled: place p of the chain is point order[p]
static void chain_case(const std::vector<int32_t> &order) {
  const size_t n = order.size();
  std::vector<float> xyz(3 * n, 0.0f), at(n);
  for (size_t p = 0; p < n; ++p) at[p] = -static_cast<float>(0.9 * kRadius * static_cast<double>(p));
  for (size_t p = 0; p < n; ++p) xyz[3 * static_cast<size_t>(order[p])] = at[p];
  std::vector<uint32_t> views(n, 1);
  std::vector<uint64_t> sum_q(n);
  for (size_t i = 0; i < n; ++i) sum_q[i] = 100 + i;
  const uint64_t step_q = cs::step_q_of(0.01f);
  const cs::HostResult res = run(xyz, views, step_q, &sum_q);
  uint64_t length = 0;  // only neighbours in the chain are linked
  for (size_t p = 1; p < n; ++p) length += cl::weight(cl::d2_of(at[p] - at[p - 1], 0.0f, 0.0f));
  const int64_t bands = static_cast<int64_t>(length / step_q) + 1;
  const int64_t nodes = static_cast<int64_t>(res.ids.size());
  expect("chain: as many nodes as bands", nodes, bands);
  expect("chain: edges", static_cast<int64_t>(res.edges.size() / 3), bands - 1);
  expect("chain: one crack", static_cast<int64_t>(res.cracks.size() / 6), 1);
  if (res.cracks.size() != 6 || nodes != bands) return;
  const int64_t want[6] = {bands, bands - 1, 2, 0, 0, 2};
  for (int k = 0; k < 6; ++k) expect("chain: summary", res.cracks[static_cast<size_t>(k)], want[k]);
  int64_t points = 0, sum_w = 0, sum_x = 0, want_x = 0;
  std::vector<int> seen(static_cast<size_t>(bands), 0);
  for (int64_t r = 0; r < nodes; ++r) {
    const int64_t *row = res.nodes.data() + 10 * r;
    expect("chain: crack row", row[0], 0);
    if (row[1] >= 0 && row[1] < bands) seen[static_cast<size_t>(row[1])] += 1;
    expect("chain: degree", row[9], (row[1] == 0 || row[1] == bands - 1) ? 1 : 2);
    expect("chain: the id is a member", res.node[static_cast<size_t>(res.ids[static_cast<size_t>(r)])], res.ids[static_cast<size_t>(r)]);
    if (r > 0) expect("chain: ids ascend", res.ids[static_cast<size_t>(r)] > res.ids[static_cast<size_t>(r - 1)], 1);
    points += row[2];
    sum_w += row[3];
    sum_x += row[6];
    expect("chain: y", row[7], 0);
    expect("chain: min <= max", row[4] <= row[5], 1);
  }
  for (int64_t b = 0; b < bands; ++b) expect("chain: one node per band", seen[static_cast<size_t>(b)], 1);
  for (size_t p = 0; p < n; ++p) want_x += cs::quant(at[p]);
  expect("chain: points", points, static_cast<int64_t>(n));
  expect("chain: widths", sum_w, static_cast<int64_t>(100 * n + n * (n - 1) / 2));
  expect("chain: quanta of x (negative)", sum_x, want_x);
  for (size_t e = 0; e + 1 < res.edges.size() / 3; ++e) {
    const int64_t *a = res.edges.data() + 3 * e, *b = a + 3;
    expect("chain: edges ascend", a[0] < b[0] || (a[0] == b[0] && a[1] < b[1]), 1);
  }
  for (size_t e = 0; e < res.edges.size() / 3; ++e) {
    const int64_t *a = res.edges.data() + 3 * e;
    expect("chain: an edge joins neighbouring bands, u the lower", res.nodes[static_cast<size_t>(10 * a[1] + 1)] - res.nodes[static_cast<size_t>(10 * a[0] + 1)], 1);
    expect("chain: one link per edge", a[2], 1);
  }
}

// the square loop of the length self-test: every weight is 4096, a = point P / 2, pos[k] = 4096 |k - P / 2|.  With a step of
// three links band 0 is one piece around a, band 16 one piece around the point opposite, and the 15 bands between two each.
static void ring_case() {
  const int side = 26, P = 4 * (side - 1);
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
  const cs::HostResult res = run(xyz, std::vector<uint32_t>(static_cast<size_t>(P), 1), 3 * 4096);
  expect("ring: one crack", static_cast<int64_t>(res.cracks.size() / 6), 1);
  if (res.cracks.size() != 6) return;
  const int64_t want[6] = {32, 32, 0, 0, 1, 2};
  for (int k = 0; k < 6; ++k) expect("ring: summary", res.cracks[static_cast<size_t>(k)], want[k]);
  for (int k = 0; k < P; ++k) {
    const int d = std::abs(k - P / 2), b = d / 3;
    // the lowest index of the piece: band 0 is 48..52, band 16 is 98, 99, 0, 1, 2
    const int lowest = b == 0 ? 48 : b == 16 ? 0 : k < P / 2 ? P / 2 - 3 * b - 2 : P / 2 + 3 * b;
    expect("ring: node", res.node[static_cast<size_t>(k)], lowest);
  }
  for (size_t r = 0; r < res.ids.size(); ++r) expect("ring: degree", res.nodes[10 * r + 9], 2);
  for (size_t e = 0; e < res.edges.size() / 3; ++e) expect("ring: links", res.edges[3 * e + 2], 1);
}

static void single_case() {
  const std::vector<float> xyz = {9.0f, 9.0f, 9.0f, -1.0f, 2.0f, 3.0f, -1.001f, 2.0f, 3.0f};
  const std::vector<uint32_t> views = {0, 1, 0};
  const std::vector<uint64_t> sum_q = {0, 777, 0};
  const cs::HostResult res = run(xyz, views, cs::step_q_of(0.01f), &sum_q);
  expect("single: one node", static_cast<int64_t>(res.ids.size()), 1);
  expect("single: no edge", static_cast<int64_t>(res.edges.size()), 0);
  if (res.ids.size() != 1 || res.cracks.size() != 6) {
    expect("single: one crack", static_cast<int64_t>(res.cracks.size() / 6), 1);
    return;
  }
  expect("single: id", res.ids[0], 1);
  const int64_t row[10] = {0, 0, 1, 777, 777, 777, -1048576, 2097152, 3145728, 0};
  for (int k = 0; k < 10; ++k) expect("single: node row", res.nodes[static_cast<size_t>(k)], row[k]);
  const int64_t crack[6] = {1, 0, 0, 0, 0, 0};
  for (int k = 0; k < 6; ++k) expect("single: summary", res.cracks[static_cast<size_t>(k)], crack[k]);
  expect("single: node of the crack point", res.node[1], 1);
  expect("single: no crack point", res.node[0], -1);
  expect("single: no crack point", res.node[2], -1);
  expect("single: centroid", cs::centroid(res.nodes[6], res.nodes[2]) == -1.0, 1);
  const cs::HostResult none = run({}, {}, cs::step_q_of(0.01f));
  expect("empty: nodes", static_cast<int64_t>(none.ids.size() + none.edges.size() + none.cracks.size() + none.node.size()), 0);
  // a crack point beyond 2^20 m is refused, a point that is no crack point there is not
  cs::HostResult far;
  const std::vector<float> out = {2.0e6f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f};
  expect("range: a crack point", cs::skeleton_brute(2, out.data(), std::vector<uint32_t>{1, 1}.data(), nullptr, 1, gn::threshold_of(kRadius), 10485, far),
         cs::kBruteRange);
  expect("range: no crack point", cs::skeleton_brute(2, out.data(), std::vector<uint32_t>{0, 1}.data(), nullptr, 1, gn::threshold_of(kRadius), 10485, far),
         cs::kBruteOk);
}

int main() {
  step_cases();
  quant_cases();
  const size_t n = 200;
  std::vector<int32_t> order(n);
  std::iota(order.begin(), order.end(), 0);
  for (size_t i = n - 1; i > 0; --i) std::swap(order[i], order[static_cast<size_t>(mix(i) % (i + 1))]);
  chain_case(order);
  ring_case();
  single_case();
  std::printf("crack_skeleton_selftest: %llu mismatches\n", (unsigned long long)bad);
  return bad ? 1 : 0;
}
