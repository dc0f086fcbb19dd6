// facets_selftest -- csrc/pcp_facets.hpp compiled for the host (CPU only: never a GPU job; meant to be built with
// -fsanitize=address,undefined as well): the cores of pcp_facets_host and pcp_facet_plane_host.  Checks the parameter rules, the
// constants of a link, the quantised normal and its record, the symmetry of the link on random pairs, the partition of a
// random scene of noisy sheets against a naive fixed point over the same links, its moments against sums taken in 128-bit
// integers, its invariance under the order of the input and under the sign of the normals, min_points, the range check and
// the plane of a tilted sheet.  Prints the number of mismatches; exit code 0 iff none.   usage: facets_selftest [points]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/pcp_facets.hpp"

using namespace pcp;

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

static float unit(uint64_t r) { return static_cast<float>(static_cast<double>(r >> 11) * (1.0 / 9007199254740992.0)); }

int main(int argc, char **argv) {
  const int64_t n = argc > 1 ? std::strtoll(argv[1], nullptr, 10) : 1200;
  uint64_t bad = 0;
  auto fail = [&](const char *what, double a, double b) {
    if (bad < 10) std::fprintf(stderr, "mismatch (%s): %.17g %.17g\n", what, a, b);
    ++bad;
  };
  // the parameter rules
  if (fa::refusal(0.1f, 10.0f, 0.01f, 0.02f, 1000) || fa::refusal(0.005f, 45.0f, 1e-4f, 0.0f, 1) || fa::refusal(1.0f, 0.5f, 0.1f, 1.0f, 1 << 24))
    fail("refusal of good parameters", 0, 0);
  if (!fa::refusal(0.004f, 10.0f, 0.01f, 0.02f, 10) || !fa::refusal(0.1f, 0.0f, 0.01f, 0.02f, 10) || !fa::refusal(0.1f, 45.5f, 0.01f, 0.02f, 10) ||
      !fa::refusal(0.1f, 10.0f, 0.2f, 0.02f, 10) || !fa::refusal(0.1f, 10.0f, 0.01f, -0.1f, 10) || !fa::refusal(0.1f, 10.0f, 0.01f, NAN, 10) ||
      !fa::refusal(0.1f, NAN, 0.01f, 0.02f, 10) || !fa::refusal(0.1f, 10.0f, 0.01f, 0.02f, 0) || !fa::refusal(0.1f, 10.0f, 0.01f, 0.02f, (1 << 24) + 1))
    fail("refusal of bad parameters", 0, 0);
  const fa::Link l = fa::link_of(0.12f, 10.0f, 0.01f);
  if (l.c_q != static_cast<int64_t>(std::ceil(std::cos(10.0 * (3.14159265358979323846 / 180.0)) * 268435456.0)) || l.c_q <= 0 || l.c_q > 268435456)
    fail("c_q", static_cast<double>(l.c_q), 0);
  if (l.t_q != static_cast<int64_t>(std::floor(static_cast<double>(0.01f) * 17179869184.0))) fail("t_q", static_cast<double>(l.t_q), 0);
  // the quantised normal and its record
  if (fa::quantise_normal(1.0f) != 16384 || fa::quantise_normal(-1.0f) != -16384 || fa::quantise_normal(0.5f / 16384.0f) != 0 ||
      fa::quantise_normal(1.5f / 16384.0f) != 2 || fa::quantise_normal(-2.5f / 16384.0f) != -2)
    fail("quantise_normal", 0, 0);
  if (fa::normal_valid(0.0f, 0.0f, 0.0f) || fa::normal_valid(NAN, 0.0f, 1.0f) || fa::normal_valid(0.0f, 1.5f, 0.0f) || !fa::normal_valid(0.0f, -1.0f, 0.0f))
    fail("normal_valid", 0, 0);
  for (int64_t k = 0; k < 20000; ++k) {
    const fa::Normal q = fa::normal_of(2.0f * unit(mix(3 * k)) - 1.0f, 2.0f * unit(mix(3 * k + 1)) - 1.0f, 2.0f * unit(mix(3 * k + 2)) - 1.0f);
    uint32_t lo, hi;
    fa::pack(q, true, &lo, &hi);
    const fa::Normal u = fa::unpack(lo, hi);
    if (u.x != q.x || u.y != q.y || u.z != q.z || !fa::record_valid(hi)) fail("record", q.x, u.x);
  }
  // a scene: four noisy sheets (two parallel 3 cm apart, one tilted by 20 degrees, one far away), normals with random signs
  std::vector<float> xyz(static_cast<size_t>(3 * n)), nrm(static_cast<size_t>(3 * n)), cur(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    const int sheet = static_cast<int>(mix(7 * i) & 3);
    const float a = unit(mix(7 * i + 1)), b = unit(mix(7 * i + 2)), e = (unit(mix(7 * i + 3)) - 0.5f) * 0.002f;
    const float sgn = (mix(7 * i + 4) & 1) ? 1.0f : -1.0f;
    float p[3] = {a, b, e}, v[3] = {0.0f, 0.0f, 1.0f};
    if (sheet == 1) p[2] += 0.03f;
    if (sheet == 2) {
      const float c = std::cos(0.34906585f), s = std::sin(0.34906585f);
      p[0] = 1.0f + a * c - e * s;
      p[2] = a * s + e * c;
      v[0] = -s;
      v[2] = c;
    }
    if (sheet == 3) p[0] += 7.0f;
    for (int k = 0; k < 3; ++k) {
      xyz[static_cast<size_t>(3 * i + k)] = p[k] + 100.0f;
      nrm[static_cast<size_t>(3 * i + k)] = sgn * v[k];
    }
    cur[static_cast<size_t>(i)] = (mix(7 * i + 5) % 50 == 0) ? 0.2f : 0.001f;  // a few points of high curvature
  }
  if (n > 10) {
    xyz[3] = NAN;                        // a non-finite point
    nrm[6] = nrm[7] = nrm[8] = 0.0f;     // an invalid normal
  }
  std::vector<int32_t> label(static_cast<size_t>(n));
  fa::Table t;
  if (!fa::partition_brute(n, xyz.data(), nrm.data(), cur.data(), l, 0.02f, 1, label.data(), t)) fail("range", t.unfit, 0);
  // symmetry of the link, and the labels against a naive fixed point over the links
  std::vector<int32_t> naive(static_cast<size_t>(n));
  std::vector<uint8_t> fp(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    fp[static_cast<size_t>(i)] = fa::facet_point(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], cur[i], 0.02f);
    naive[static_cast<size_t>(i)] = fp[static_cast<size_t>(i)] ? static_cast<int32_t>(i) : -1;
  }
  std::vector<std::pair<int32_t, int32_t>> edges;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = i + 1; j < n; ++j) {
      if (!fp[static_cast<size_t>(i)] || !fp[static_cast<size_t>(j)]) continue;
      const fa::Normal ni = fa::normal_of(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]), nj = fa::normal_of(nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2]);
      const bool ij = fa::linked(xyz[3 * j] - xyz[3 * i], xyz[3 * j + 1] - xyz[3 * i + 1], xyz[3 * j + 2] - xyz[3 * i + 2], ni, nj, l);
      const bool ji = fa::linked(xyz[3 * i] - xyz[3 * j], xyz[3 * i + 1] - xyz[3 * j + 1], xyz[3 * i + 2] - xyz[3 * j + 2], nj, ni, l);
      if (ij != ji) fail("symmetry", static_cast<double>(i), static_cast<double>(j));
      if (ij) edges.emplace_back(static_cast<int32_t>(i), static_cast<int32_t>(j));
    }
  for (bool moved = true; moved;) {
    moved = false;
    for (const auto &e : edges) {
      const int32_t lo = std::min(naive[static_cast<size_t>(e.first)], naive[static_cast<size_t>(e.second)]);
      if (naive[static_cast<size_t>(e.first)] != lo || naive[static_cast<size_t>(e.second)] != lo) {
        naive[static_cast<size_t>(e.first)] = naive[static_cast<size_t>(e.second)] = lo;
        moved = true;
      }
    }
  }
  for (int64_t i = 0; i < n; ++i)
    if (naive[static_cast<size_t>(i)] != label[static_cast<size_t>(i)]) fail("labels", naive[static_cast<size_t>(i)], label[static_cast<size_t>(i)]);
  if (n > 10 && (label[1] != -1 || label[2] != -1)) fail("non-finite point or invalid normal labelled", label[1], label[2]);
  if (n >= 1200 && t.ids.size() < 4) fail("the four sheets", static_cast<double>(t.ids.size()), 4);
  // the rows against 128-bit sums and the box against the members
  for (size_t r = 0; r < t.ids.size(); ++r) {
    const int32_t id = t.ids[r];
    __int128 s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    cf::Box b;
    cf::clear(b);
    for (int64_t i = 0; i < n; ++i) {
      if (label[static_cast<size_t>(i)] != id) continue;
      const __int128 x = fa::moment_q(xyz[3 * i] - xyz[3 * id]), y = fa::moment_q(xyz[3 * i + 1] - xyz[3 * id + 1]),
                     z = fa::moment_q(xyz[3 * i + 2] - xyz[3 * id + 2]);
      const __int128 add[10] = {1, x, y, z, x * x, x * y, x * z, y * y, y * z, z * z};
      for (int a = 0; a < 10; ++a) s[a] += add[a];
      cf::add(b, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    }
    for (int a = 0; a < 10; ++a)
      if (static_cast<__int128>(t.rows[10 * r + a]) != s[a]) fail("row", static_cast<double>(t.rows[10 * r + a]), static_cast<double>(s[a]));
    for (int a = 0; a < 3; ++a)
      if (t.box[6 * r + a] != b.lo[a] || t.box[6 * r + 3 + a] != b.hi[a]) fail("box", static_cast<double>(r), a);
    if (r > 0 && t.ids[r - 1] >= id) fail("ids ascend", t.ids[r - 1], id);
  }
  // the input reversed with every normal negated: the same partition (labels are lowest indices of the NEW order)
  {
    std::vector<float> rx(xyz.size()), rn(nrm.size()), rc(cur.size());
    for (int64_t i = 0; i < n; ++i) {
      for (int k = 0; k < 3; ++k) {
        rx[static_cast<size_t>(3 * i + k)] = xyz[static_cast<size_t>(3 * (n - 1 - i) + k)];
        rn[static_cast<size_t>(3 * i + k)] = -nrm[static_cast<size_t>(3 * (n - 1 - i) + k)];
      }
      rc[static_cast<size_t>(i)] = cur[static_cast<size_t>(n - 1 - i)];
    }
    std::vector<int32_t> rl(static_cast<size_t>(n));
    fa::Table rt;
    if (!fa::partition_brute(n, rx.data(), rn.data(), rc.data(), l, 0.02f, 1, rl.data(), rt)) fail("range (reversed)", rt.unfit, 0);
    if (rt.ids.size() != t.ids.size()) fail("facets (reversed)", static_cast<double>(rt.ids.size()), static_cast<double>(t.ids.size()));
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j : {(i * 7 + 3) % n, (i * 13 + 5) % n}) {
        const bool same = label[static_cast<size_t>(i)] >= 0 && label[static_cast<size_t>(i)] == label[static_cast<size_t>(j)];
        const bool rsame = rl[static_cast<size_t>(n - 1 - i)] >= 0 && rl[static_cast<size_t>(n - 1 - i)] == rl[static_cast<size_t>(n - 1 - j)];
        if (same != rsame || (label[static_cast<size_t>(i)] < 0) != (rl[static_cast<size_t>(n - 1 - i)] < 0)) fail("order of the input", static_cast<double>(i), static_cast<double>(j));
      }
  }
  // min_points on both sides of the largest facet's size
  if (!t.ids.empty()) {
    int64_t most = 0;
    for (size_t r = 0; r < t.ids.size(); ++r) most = std::max<int64_t>(most, t.rows[10 * r]);
    fa::Table a, b;
    std::vector<int32_t> la(static_cast<size_t>(n)), lb(static_cast<size_t>(n));
    fa::partition_brute(n, xyz.data(), nrm.data(), cur.data(), l, 0.02f, static_cast<int32_t>(most), la.data(), a);
    fa::partition_brute(n, xyz.data(), nrm.data(), cur.data(), l, 0.02f, static_cast<int32_t>(most + 1), lb.data(), b);
    if (a.ids.empty() || !b.ids.empty() || a.components != t.components || b.facet_points != t.facet_points) fail("min_points", static_cast<double>(a.ids.size()), static_cast<double>(b.ids.size()));
    for (int64_t i = 0; i < n; ++i)
      if (lb[static_cast<size_t>(i)] != -1) fail("min_points labels", static_cast<double>(i), lb[static_cast<size_t>(i)]);
  }
  // the range check: a facet that wide cannot be made of 65536 linked points, so the check is asked directly
  {
    const uint32_t wide[6] = {cf::order_bits(0.0f), cf::order_bits(0.0f), cf::order_bits(0.0f), cf::order_bits(300000.0f), cf::order_bits(1.0f), cf::order_bits(1.0f)};
    const uint32_t room[6] = {cf::order_bits(-6.0f), cf::order_bits(-5.0f), cf::order_bits(0.0f), cf::order_bits(6.0f), cf::order_bits(5.0f), cf::order_bits(4.0f)};
    if (fa::moments_fit(1000, wide) || !fa::moments_fit(1 << 24, room) || !fa::moments_fit(1, wide)) fail("moments_fit", 0, 0);
  }
  // the plane of a sheet tilted by 30 degrees about y, 0.5 mm of noise along its normal: normal, centroid and rms
  {
    const double c = std::cos(0.5235987755982988), s = std::sin(0.5235987755982988);
    const int64_t m = 4000;
    std::vector<float> p(static_cast<size_t>(3 * m));
    long double sum[3] = {0, 0, 0}, e2 = 0;
    for (int64_t i = 0; i < m; ++i) {
      const double a = unit(mix(11 * i + 1)) - 0.5, b = unit(mix(11 * i + 2)) - 0.5, e = (unit(mix(11 * i + 3)) - 0.5) * 0.001;
      p[static_cast<size_t>(3 * i)] = static_cast<float>(5.0 + a * c - e * s);
      p[static_cast<size_t>(3 * i + 1)] = static_cast<float>(-3.0 + b);
      p[static_cast<size_t>(3 * i + 2)] = static_cast<float>(2.0 + a * s + e * c);
      for (int k = 0; k < 3; ++k) sum[k] += p[static_cast<size_t>(3 * i + k)];
      e2 += e * e;
    }
    int64_t row[10] = {m, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = 0; i < m; ++i) fa::add_member(row, fa::moment_q(p[static_cast<size_t>(3 * i)] - p[0]), fa::moment_q(p[static_cast<size_t>(3 * i + 1)] - p[1]), fa::moment_q(p[static_cast<size_t>(3 * i + 2)] - p[2]));
    double out[7];
    if (!fa::plane_of(p.data(), row, out)) fail("plane_of", 0, 0);
    for (int k = 0; k < 3; ++k)
      if (std::fabs(out[k] - static_cast<double>(sum[k] / m)) > 1.3e-4) fail("centroid", out[k], static_cast<double>(sum[k] / m));  // (half a quantum)
    if (std::fabs(out[3] + s) > 1e-3 || std::fabs(out[4]) > 1e-3 || std::fabs(out[5] - c) > 1e-3) fail("normal", out[3], out[5]);
    const double rms = std::sqrt(static_cast<double>(e2 / m));
    if (!(out[6] > 0.8 * rms && out[6] < 1.3 * rms)) fail("rms", out[6], rms);
    const int64_t none[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, one[10] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (fa::plane_of(p.data(), none, out)) fail("plane of no point", 0, 0);
    if (!fa::plane_of(p.data(), one, out) || out[3] != 0.0 || out[4] != 0.0 || out[5] != 0.0 || out[6] != 0.0 || out[0] != static_cast<double>(p[0]))
      fail("plane of one point", out[3], out[6]);
  }
  std::printf("%llu mismatches\n", static_cast<unsigned long long>(bad));
  return bad ? 1 : 0;
}
