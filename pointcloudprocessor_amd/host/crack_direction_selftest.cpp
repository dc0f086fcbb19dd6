// crack_direction_selftest -- csrc/pcp_crack_direction.hpp compiled for the host (CPU only: never a GPU job; meant to be built
// with -fsanitize=address,undefined as well).  The parameter rules the entry points share, a three-point line worked by hand,
// the zero S1 sums of every crack, the (lo, hi) split of a word near +-2^62 and of sums beyond 2^63, the sign rule, the
// degenerate pairs, the axis of hand-made rows, and a checksum over the integers of a fixed seeded cloud.  Prints the number of
// mismatches; exit code 0 iff none.   usage: crack_direction_selftest
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../csrc/pcp_crack_direction.hpp"

using namespace pcp;

static uint64_t bad = 0;
static void expect(const char *what, int64_t got, int64_t want) {
  if (got == want) return;
  if (bad < 10) std::fprintf(stderr, "mismatch (%s): %lld, expected %lld\n", what, (long long)got, (long long)want);
  ++bad;
}
static void near(const char *what, double got, double want, double tol) {
  if (std::fabs(got - want) <= tol) return;
  if (bad < 10) std::fprintf(stderr, "mismatch (%s): %.17g, expected %.17g\n", what, got, want);
  ++bad;
}

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

constexpr float kRadius = 0.005f;

static cd::HostResult run(const std::vector<float> &xyz, const std::vector<uint32_t> &views, int32_t min_views = 1) {
  cd::HostResult res;
  if (!cd::directions_brute(static_cast<int64_t>(views.size()), xyz.data(), views.data(), min_views, gn::threshold_of(kRadius), res))
    expect("directions_brute: no point has 2^22 links", 0, 1);
  return res;
}

static void parameter_cases() {
  expect("min_views 0", cf::min_views_ok(0), 0);
  expect("min_views 1", cf::min_views_ok(1), 1);
  expect("min_views 4096", cf::min_views_ok(4096), 1);
  expect("min_views 4097", cf::min_views_ok(4097), 0);
  expect("radius 0.005", gn::radius_ok(0.005f), 1);
  expect("radius below 0.005", gn::radius_ok(std::nextafter(0.005f, 0.0f)), 0);
  expect("radius 1", gn::radius_ok(1.0f), 1);
  expect("radius above 1", gn::radius_ok(std::nextafter(1.0f, 2.0f)), 0);
  expect("radius NaN", gn::radius_ok(std::nanf("")), 0);
  expect("row words", cd::kRowWords, 20);
}

// three points on the x axis, 2^-8 m apart (d2 = 2^-16 < t; the outer two are 2^-7 apart: not linked); point 3 is far away and
// point 4 has no view.  q = 2^12 per link.
static void line_case() {
  const float h = 1.0f / 256.0f;
  const std::vector<float> xyz = {1.0f, 2.0f, 3.0f, 1.0f + h, 2.0f, 3.0f, 1.0f + 2 * h, 2.0f, 3.0f, 9.0f, 9.0f, 9.0f, 1.0f + h, 2.0f, 3.0f};
  const cd::HostResult res = run(xyz, {1, 1, 1, 1, 0});
  const int64_t q = 4096, qq = q * q;
  const int64_t want[5][10] = {{1, q, 0, 0, qq, 0, 0, 0, 0, 0}, {2, 0, 0, 0, 2 * qq, 0, 0, 0, 0, 0}, {1, -q, 0, 0, qq, 0, 0, 0, 0, 0},
                               {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
  for (size_t i = 0; i < 5; ++i) {
    expect("line: links", res.links[i], want[i][0]);
    for (size_t k = 0; k < 10; ++k) expect("line: moments", res.moments[10 * i + k], want[i][k]);
  }
  // only the middle point has two links: C = diag(2 q^2, 0, 0), tangent (1, 0, 0), anisotropy 1
  const float tangent[5][3] = {{0, 0, 0}, {1, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (size_t i = 0; i < 5; ++i) {
    for (size_t a = 0; a < 3; ++a) expect("line: tangent", res.tangent[3 * i + a] == tangent[i][a], 1);
    expect("line: anisotropy", res.anisotropy[i] == (i == 1 ? 1.0f : 0.0f), 1);
  }
  expect("line: cracks", static_cast<int64_t>(res.ids.size()), 2);
  if (res.ids.size() != 2) return;
  expect("line: id 0", res.ids[0], 0);
  expect("line: id 1", res.ids[1], 3);
  const int64_t row0[20] = {4, 0, 0, 0, 0, 0, 0, 0, 4 * qq, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // (S1x: lo 2^32, hi -1, see split_cases)
  for (size_t k = 0; k < 20; ++k)
    if (k != 2 && k != 3) expect("line: row 0", res.rows[k], row0[k]);
  expect("line: S1x of row 0", res.rows[3] * 4294967296ll + res.rows[2], 0);
  for (size_t k = 0; k < 20; ++k) expect("line: the lone point's row", res.rows[20 + k], 0);
  double out5[5];
  cd::axis_host(res.rows.data(), out5);
  near("line: L", out5[0], 4.0, 0.0);
  near("line: axis x", out5[1], 1.0, 0.0);
  near("line: axis y", out5[2], 0.0, 0.0);
  near("line: axis z", out5[3], 0.0, 0.0);
  near("line: axis anisotropy", out5[4], 1.0, 0.0);
  cd::axis_host(res.rows.data() + 20, out5);
  for (int k = 0; k < 5; ++k) near("line: no axis without links", out5[k], 0.0, 0.0);
}

static void split_cases() {
  for (const int64_t v : {int64_t(0), int64_t(1), int64_t(-1), (int64_t(1) << 62) - 3, -(int64_t(1) << 62) + 3, (int64_t(1) << 32), -(int64_t(1) << 32),
                          int64_t(0xffffffffll), int64_t(-4096)}) {
    const uint64_t lo = cd::lo_of(v);
    const int64_t hi = cd::hi_of(v);
    expect("split: lo < 2^32", lo < (1ull << 32), 1);
    expect("split: hi * 2^32 + lo", static_cast<int64_t>(static_cast<uint64_t>(hi) * (1ull << 32) + lo), v);
  }
  expect("split: hi of 2^62 - 3", cd::hi_of((int64_t(1) << 62) - 3), (int64_t(1) << 30) - 1);
  expect("split: lo of 2^62 - 3", static_cast<int64_t>(cd::lo_of((int64_t(1) << 62) - 3)), 0xfffffffdll);
  expect("split: hi of -2^62 + 3", cd::hi_of(-(int64_t(1) << 62) + 3), -(int64_t(1) << 30));
  expect("split: lo of -2^62 + 3", static_cast<int64_t>(cd::lo_of(-(int64_t(1) << 62) + 3)), 3);
  expect("split: hi of -4096", cd::hi_of(-4096), -1);
  expect("split: lo of -4096", static_cast<int64_t>(cd::lo_of(-4096)), 0xfffff000ll);
  // six words of 2^62 - 3 sum beyond 2^63 in value; the halves do not notice
  uint64_t lo = 0;
  int64_t hi = 0;
  for (int k = 0; k < 6; ++k) {
    lo += cd::lo_of((int64_t(1) << 62) - 3);
    hi += cd::hi_of((int64_t(1) << 62) - 3);
  }
  near("split: the value of a sum beyond 2^63", cd::value_of(static_cast<int64_t>(lo), hi), 6.0 * 4611686018427387904.0, 4096.0);
  near("value_of(lo 5, hi -1)", cd::value_of(5, -1), -4294967291.0, 0.0);
}

static void vector_cases() {
  double v[3] = {-0.6, 0.0, 0.8};
  cd::orient(v);
  expect("orient: the largest component decides", v[2] == 0.8 && v[0] == -0.6, 1);
  double w[3] = {-0.5, 0.5, -0.5};
  cd::orient(w);
  expect("orient: a tie goes to the lowest axis", w[0] == 0.5 && w[1] == -0.5 && w[2] == 0.5, 1);
  // C isotropic in the plane z = 0: l1 = l2, every cross product vanishes, the vector is still a unit eigenvector in the plane
  double C[6] = {7.0, 0.0, 0.0, 7.0, 0.0, 0.0}, u[3], an;
  expect("degenerate: valid", cd::largest_pair_host(C, u, &an), 1);
  near("degenerate: unit", (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2], 1.0, 1e-15);
  near("degenerate: in the plane", u[2], 0.0, 0.0);
  near("degenerate: anisotropy", an, 0.5, 1e-8);  // (a double root of the closed form: half the digits)
  double S[6] = {3.0, 0.0, 0.0, 3.0, 0.0, 3.0};
  expect("isotropic: valid", cd::largest_pair_host(S, u, &an), 1);
  near("isotropic: unit", (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2], 1.0, 1e-15);
  near("isotropic: anisotropy", an, 1.0 / 3.0, 1e-8);
  double Z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  expect("zero: invalid", cd::largest_pair_host(Z, u, &an), 0);
  expect("zero: zeros", u[0] == 0.0 && u[1] == 0.0 && u[2] == 0.0 && an == 0.0, 1);
  // a known pair: C = [[2, 1, 0], [1, 2, 0], [0, 0, 1]]: l1 = 3 along (1, 1, 0) / sqrt 2, trace 5
  double K[6] = {2.0, 1.0, 0.0, 2.0, 0.0, 1.0};
  expect("known: valid", cd::largest_pair_host(K, u, &an), 1);
  near("known: x", u[0], std::sqrt(0.5), 1e-14);
  near("known: y", u[1], std::sqrt(0.5), 1e-14);
  near("known: z", u[2], 0.0, 1e-14);
  near("known: anisotropy", an, 0.6, 1e-14);
}

// 600 seeded points in a cube sized for ~5 links each, every seventh without a view: S1 of every row is zero, the rows are the
// sums of the members' words, and the integers have one value
static void cloud_case() {
  const size_t n = 600;
  std::vector<float> xyz(3 * n);
  std::vector<uint32_t> views(n);
  for (size_t i = 0; i < n; ++i) {
    for (size_t a = 0; a < 3; ++a) xyz[3 * i + a] = static_cast<float>(static_cast<double>(mix(3 * i + a) >> 11) * (1.0 / 9007199254740992.0) * 0.04);
    views[i] = i % 7 == 3 ? 0 : 1 + static_cast<uint32_t>(mix(1000 + i) % 3);
  }
  const cd::HostResult res = run(xyz, views);
  std::vector<int32_t> label(n);
  cf::label_brute(static_cast<int64_t>(n), xyz.data(), views.data(), 1, gn::threshold_of(kRadius), label.data());
  const size_t rows = res.ids.size();
  std::vector<int64_t> value(10 * rows, 0);  // the sums as plain 64-bit words (these are small)
  int64_t valid = 0, most = 0;
  uint64_t sum = 0;
  for (size_t i = 0; i < n; ++i) {
    if (label[i] < 0) {
      for (size_t k = 0; k < 10; ++k) expect("cloud: zeros for a point that is no crack point", res.moments[10 * i + k], 0);
      continue;
    }
    size_t r = 0;
    while (res.ids[r] != label[i]) ++r;
    for (size_t k = 0; k < 10; ++k) {
      value[10 * r + k] += res.moments[10 * i + k];
      sum = mix(sum ^ static_cast<uint64_t>(res.moments[10 * i + k]));
    }
    const float *t = &res.tangent[3 * i];
    const bool has = t[0] != 0.0f || t[1] != 0.0f || t[2] != 0.0f;
    valid += has ? 1 : 0;
    most = std::max<int64_t>(most, res.links[i]);
    if (has) near("cloud: unit tangent", std::sqrt((double(t[0]) * t[0] + double(t[1]) * t[1]) + double(t[2]) * t[2]), 1.0, 1e-6);
    if (has) expect("cloud: anisotropy in (1/3, 1]", res.anisotropy[i] > 0.333f && res.anisotropy[i] <= 1.0f, 1);
    if (!has) expect("cloud: no tangent, no anisotropy", res.anisotropy[i] == 0.0f, 1);
    if (res.links[i] < 2) expect("cloud: fewer than two links, no tangent", has, 0);
  }
  for (size_t r = 0; r < rows; ++r)
    for (size_t k = 0; k < 10; ++k) {
      const int64_t v = static_cast<int64_t>(static_cast<uint64_t>(res.rows[20 * r + 2 * k + 1]) * (1ull << 32) + static_cast<uint64_t>(res.rows[20 * r + 2 * k]));
      expect("cloud: hi * 2^32 + lo = the sum of the members' words", v, value[10 * r + k]);
      if (k >= 1 && k <= 3) expect("cloud: S1 of a crack is zero", v, 0);
      expect("cloud: lo is a sum of non-negative halves", res.rows[20 * r + 2 * k] >= 0, 1);
    }
  expect("cloud: cracks", static_cast<int64_t>(rows), 36);
  expect("cloud: points with a tangent", valid, 443);
  expect("cloud: most links", most, 10);
  expect("cloud: checksum of the moments", static_cast<int64_t>(sum >> 1), 5790982894403439790ll);
}

int main() {
  parameter_cases();
  line_case();
  split_cases();
  vector_cases();
  cloud_case();
  std::printf("crack_direction_selftest: %llu mismatches\n", (unsigned long long)bad);
  return bad ? 1 : 0;
}
