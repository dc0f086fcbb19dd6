// crack_branch_selftest -- csrc/pcp_crack_branch.hpp compiled for the host (CPU only: never a GPU job; meant to be built with
// -fsanitize=address,undefined as well).  Known answers of CB1 at its boundary (0 and 1024 are taken; the float above 1024, a
// negative value, NaN and infinity are not), and of the whole stage on a 200-point chain in shuffled order (one branch, no
// attachment, as many nodes as bands), the lattice square ring of the skeleton self-test (one closed branch), a lattice T with
// a stub of two bands at `prune` below, at and above the stub's nodes * step_q (kept, kept, pruned: the comparison is strict,
// and the junction dissolves), a T whose stub holds end b (never pruned), two adjacent junctions (one bridge, no branch lost)
// and a one-point crack.  Prints the number of mismatches; exit code 0 iff none.   usage: crack_branch_selftest
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <vector>

#include "../csrc/pcp_crack_branch.hpp"

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
constexpr uint64_t kLink = 4096;         // the weight of a lattice link of 1 / 256 m
constexpr uint64_t kStepQ = 3 * kLink;   // three lattice links per band

static void prune_cases() {
  expect("prune = 0", cb::prune_ok(0.0f), 1);
  expect("prune = -0", cb::prune_ok(-0.0f), 1);
  expect("prune = 1024", cb::prune_ok(1024.0f), 1);
  expect("prune above 1024", cb::prune_ok(std::nextafter(1024.0f, 2048.0f)), 0);
  expect("prune < 0", cb::prune_ok(-std::numeric_limits<float>::denorm_min()), 0);
  expect("prune = NaN", cb::prune_ok(std::numeric_limits<float>::quiet_NaN()), 0);
  expect("prune = inf", cb::prune_ok(std::numeric_limits<float>::infinity()), 0);
  expect("prune_q(0)", static_cast<int64_t>(cb::prune_q_of(0.0f)), 0);
  expect("prune_q(1024)", static_cast<int64_t>(cb::prune_q_of(1024.0f)), int64_t(1) << 30);
  expect("prune_q(0.05)", static_cast<int64_t>(cb::prune_q_of(0.05f)), 52428);  // 0.05f * 2^20 = 52428.8
  expect("prune_q truncates", static_cast<int64_t>(cb::prune_q_of(std::nextafter(1.0f, 0.0f))), 1048575);
}

static cb::HostResult run(const std::vector<float> &xyz, const std::vector<uint32_t> &views, uint64_t step_q, uint64_t prune_q,
                          const std::vector<uint64_t> *sum_q = nullptr) {
  cb::HostResult res;
  const cb::Brute how = cb::branches_brute(static_cast<int64_t>(views.size()), xyz.data(), views.data(), sum_q ? sum_q->data() : nullptr, 1,
                                           gn::threshold_of(kRadius), step_q, prune_q, res);
  expect("the stage runs", how, cb::kBruteOk);
  return res;
}

static void expect_row(const char *what, const cb::HostResult &res, size_t b, int64_t nodes, int64_t edges_inside, int64_t attachments) {
  if (b >= res.ids.size()) return expect(what, static_cast<int64_t>(res.ids.size()), static_cast<int64_t>(b) + 1);
  const int64_t *row = res.rows.data() + cb::kRowWords * b;
  expect(what, row[1], nodes);
  expect(what, row[2], edges_inside);
  expect(what, row[3], attachments);
  expect(what, row[4] >= 0, attachments >= 1);
  expect(what, row[5] >= 0, attachments == 2);
  for (int k = 1; k <= 3; ++k)  // CB6: the value hi * 2^32 + lo
    expect("S1 sums are zero", res.moments[cd::kRowWords * b + 2 * k] + res.moments[cd::kRowWords * b + 2 * k + 1] * 4294967296ll, 0);
}

static void expect_cracks(const char *what, const cb::HostResult &res, const int64_t (&want)[7]) {
  expect(what, static_cast<int64_t>(res.cracks.size()), 7);
  if (res.cracks.size() != 7) return;
  for (int k = 0; k < 7; ++k) expect(what, res.cracks[static_cast<size_t>(k)], want[k]);
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
  uint64_t length = 0;  // only neighbours in the chain are linked
  for (size_t p = 1; p < n; ++p) length += cl::weight(cl::d2_of(at[p] - at[p - 1], 0.0f, 0.0f));
  const int64_t bands = static_cast<int64_t>(length / step_q) + 1;
  for (uint64_t prune_q : {uint64_t(0), uint64_t(1) << 30}) {  // no junction: nothing to prune whatever the bound
    const cb::HostResult res = run(xyz, views, step_q, prune_q, &sum_q);
    expect("chain: one branch", static_cast<int64_t>(res.ids.size()), 1);
    expect_row("chain: the branch", res, 0, bands, bands - 1, 0);
    expect_cracks("chain: summary", res, {1, 0, 0, 2, 0, 0, 0});
    if (res.ids.size() != 1) continue;
    expect("chain: id", res.ids[0], 0);
    const int64_t *row = res.rows.data();
    expect("chain: points", row[6], static_cast<int64_t>(n));
    expect("chain: widths", row[7], static_cast<int64_t>(100 * n + n * (n - 1) / 2));
    expect("chain: min_w", row[8], 100);
    expect("chain: max_w", row[9], static_cast<int64_t>(99 + n));
    expect("chain: pos_min", row[10], 0);
    expect("chain: pos_max", row[11], static_cast<int64_t>(length));
    expect("chain: ordered links", res.moments[0], static_cast<int64_t>(2 * (n - 1)));
    for (size_t i = 0; i < n; ++i) expect("chain: branch[]", res.branch[i], 0);
    for (int32_t e : res.edge_branch) expect("chain: edge_branch", e, 0);
    expect("chain: edges", static_cast<int64_t>(res.edge_branch.size()), bands - 1);
  }
}

static void lattice(std::vector<float> &xyz, int x, int y) {
  xyz.push_back(static_cast<float>(x) / 256.0f);
  xyz.push_back(static_cast<float>(y) / 256.0f);
  xyz.push_back(0.25f);
}

// the square loop of the skeleton self-test: 32 nodes and 32 edges, no junction
static void ring_case() {
  const int side = 26, P = 4 * (side - 1);
  std::vector<float> xyz;
  for (int k = 0; k < P; ++k) {
    const int e = k / (side - 1), o = k % (side - 1);
    lattice(xyz, e == 0 ? o : e == 1 ? side - 1 : e == 2 ? side - 1 - o : 0, e == 0 ? 0 : e == 1 ? o : e == 2 ? side - 1 : side - 1 - o);
  }
  const cb::HostResult res = run(xyz, std::vector<uint32_t>(static_cast<size_t>(P), 1), kStepQ, cb::prune_q_of(1.0f));
  expect("ring: one branch", static_cast<int64_t>(res.ids.size()), 1);
  expect_row("ring: a closed branch", res, 0, 32, 32, 0);
  expect_cracks("ring: summary", res, {1, 0, 0, 0, 0, 0, 0});
}

// A stem of 31 lattice points along x (point x is index x) and stubs of six points at right angles from the stem points in
// `at`, upwards and downwards in turn.  The first sweep of CL4 starts at index 0, so end a is x = 30 and pos = 4096 * (30 - x) on
// the stem.  A stub leaves where 30 - x = 2 mod 3, the last point of its band: its first point opens the next band and is not
// linked to the stem point of that band (a diagonal of the lattice is longer than the radius), so the stub is two nodes of three
// points and the band of its foot a node of degree 3.
static std::vector<float> tee(const std::vector<int> &at) {
  std::vector<float> xyz;
  for (int x = 0; x <= 30; ++x) lattice(xyz, x, 0);
  for (size_t k = 0; k < at.size(); ++k)
    for (int y = 1; y <= 6; ++y) lattice(xyz, at[k], k % 2 ? -y : y);
  return xyz;
}

static void tee_case() {
  const std::vector<float> xyz = tee({13});  // pos of the foot 17: band 5 of 0..10
  const std::vector<uint32_t> views(37, 1);
  const uint64_t stub_q = 2 * kStepQ;  // the stub's nodes * step_q
  for (int k = -1; k <= 1; ++k) {
    const cb::HostResult res = run(xyz, views, kStepQ, stub_q + static_cast<uint64_t>(k));
    if (k <= 0) {  // below and at: kept (the comparison is strict)
      expect("T kept: branches", static_cast<int64_t>(res.ids.size()), 3);
      expect_cracks("T kept: summary", res, {3, 0, 1, 3, 0, 0, 0});
      if (res.ids.size() != 3) continue;
      expect("T kept: ids", res.ids[0] == 0 && res.ids[1] == 16 && res.ids[2] == 31, 1);
      expect_row("T kept: the far side (x < 13)", res, 0, 5, 4, 1);
      expect_row("T kept: the side of end a", res, 1, 5, 4, 1);
      expect_row("T kept: the stub", res, 2, 2, 1, 1);
      for (int x = 13; x <= 15; ++x) expect("T kept: the junction's points", res.branch[static_cast<size_t>(x)], cb::kJunction);
      expect("T kept: all three attach to one junction", res.rows[4] == res.rows[cb::kRowWords + 4] && res.rows[4] == res.rows[2 * cb::kRowWords + 4], 1);
      expect("T kept: stub points", res.rows[2 * cb::kRowWords + 6], 6);
      expect("T kept: stub pos_min", res.rows[2 * cb::kRowWords + 10], 18 * 4096);
      expect("T kept: stub pos_max", res.rows[2 * cb::kRowWords + 11], 23 * 4096);
    } else {  // above: pruned, the junction dissolves and the two sides come out as one branch
      expect("T pruned: branches", static_cast<int64_t>(res.ids.size()), 1);
      expect_cracks("T pruned: summary", res, {1, 0, 0, 2, 1, 2, 6});
      expect_row("T pruned: the stem", res, 0, 11, 10, 0);
      expect("T pruned: pruned_branches", res.pruned_branches, 1);
      for (int i = 0; i < 37; ++i) expect("T pruned: branch[]", res.branch[static_cast<size_t>(i)], i < 31 ? 0 : cb::kPruned);
      int64_t pruned_edges = 0;
      for (int32_t e : res.edge_branch) pruned_edges += e == cb::kEdgePruned;
      expect("T pruned: edges with a pruned end", pruned_edges, 2);
      if (res.ids.size() == 1) expect("T pruned: points", res.rows[6], 31);
    }
  }
}

// the stub at x = 4 (pos of the foot 26): its tip is 32 links from end a, the stem's end at x = 0 only 30, so the stub holds
// end b; the two nodes the stem has left past the foot are a spur and go, the stub stays
static void end_case() {
  const std::vector<float> xyz = tee({4});
  const cb::HostResult res = run(xyz, std::vector<uint32_t>(37, 1), kStepQ, 2 * kStepQ + 1);
  expect("end b in the stub: branches", static_cast<int64_t>(res.ids.size()), 1);
  expect_cracks("end b in the stub: summary", res, {1, 0, 0, 2, 1, 2, 4});
  for (int i = 0; i < 37; ++i) expect("end b in the stub: branch[]", res.branch[static_cast<size_t>(i)], i < 4 ? cb::kPruned : 4);
  if (res.ids.size() == 1) expect("end b in the stub: pos_max", res.rows[11], 32 * 4096);
}

// stubs at x = 13 (up) and x = 10 (down): their feet are bands 5 and 6, two junctions joined by one bridge
static void bridge_case() {
  const std::vector<float> xyz = tee({13, 10});
  const cb::HostResult res = run(xyz, std::vector<uint32_t>(43, 1), kStepQ, 0);
  expect("bridge: branches", static_cast<int64_t>(res.ids.size()), 4);
  expect_cracks("bridge: summary", res, {4, 1, 2, 4, 0, 0, 0});
  int64_t bridges = 0, nodes = 0;
  for (int32_t e : res.edge_branch) bridges += e == cb::kBridge;
  expect("bridge: one edge is a bridge", bridges, 1);
  for (size_t b = 0; b < res.ids.size(); ++b) {
    nodes += res.rows[cb::kRowWords * b + 1];
    expect("bridge: attachments", res.rows[cb::kRowWords * b + 3], 1);
  }
  expect("bridge: no node lost", nodes + 2, 15);
  int64_t junction_points = 0;
  for (int32_t b : res.branch) junction_points += b == cb::kJunction;
  expect("bridge: the points of two junctions", junction_points, 6);
}

static void single_case() {
  const std::vector<float> xyz = {9.0f, 9.0f, 9.0f, -1.0f, 2.0f, 3.0f, -1.001f, 2.0f, 3.0f};
  const std::vector<uint32_t> views = {0, 1, 0};
  const std::vector<uint64_t> sum_q = {0, 777, 0};
  const cb::HostResult res = run(xyz, views, cs::step_q_of(0.01f), cb::prune_q_of(1024.0f), &sum_q);
  expect("single: one branch", static_cast<int64_t>(res.ids.size()), 1);
  expect_cracks("single: summary", res, {1, 0, 0, 0, 0, 0, 0});
  if (res.ids.size() != 1) return;
  expect("single: id", res.ids[0], 1);
  const int64_t row[15] = {0, 1, 0, 0, -1, -1, 1, 777, 777, 777, 0, 0, -1048576, 2097152, 3145728};
  for (int k = 0; k < 15; ++k) expect("single: row", res.rows[static_cast<size_t>(k)], row[k]);
  for (int k = 0; k < 20; ++k) expect("single: no link", res.moments[static_cast<size_t>(k)], 0);
  expect("single: branch of the crack point", res.branch[1], 1);
  expect("single: no crack point", res.branch[0], cb::kNoPoint);
  expect("single: no crack point", res.branch[2], cb::kNoPoint);
  const cb::HostResult none = run({}, {}, cs::step_q_of(0.01f), 0);
  expect("empty", static_cast<int64_t>(none.ids.size() + none.rows.size() + none.cracks.size() + none.branch.size() + none.edge_branch.size()), 0);
}

int main() {
  prune_cases();
  const size_t n = 200;
  std::vector<int32_t> order(n);
  std::iota(order.begin(), order.end(), 0);
  for (size_t i = n - 1; i > 0; --i) std::swap(order[i], order[static_cast<size_t>(mix(i) % (i + 1))]);
  chain_case(order);
  ring_case();
  tee_case();
  end_case();
  bridge_case();
  single_case();
  std::printf("crack_branch_selftest: %llu mismatches\n", (unsigned long long)bad);
  return bad ? 1 : 0;
}
