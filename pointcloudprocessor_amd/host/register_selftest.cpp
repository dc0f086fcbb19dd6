// register_selftest -- csrc/pcp_register.hpp compiled for the host (CPU only: never a GPU job; meant to be built with
// -fsanitize=address,undefined as well).  Checks the parameters' bounds, the transform (identity, the fixed sequence against
// long double, the 4 x 4 and back), the match key's order and tie rule, the normal's test, the lever arm's rounding and range,
// the trim's boundary, the thirty terms and their halves against 128-bit arithmetic at the widest ranges, the sums' invariance
// under the order of the pairs, the solve at rank 6, 3 and 0 (a planted update is recovered, unobservable components stay
// exactly zero), a sum that needs both halves, the composition and the loop's three endings.  Prints the number of
// mismatches; exit code 0 iff none.
//   usage: register_selftest [pairs]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/pcp_register.hpp"

using namespace pcp;

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

static double unit(uint64_t r) { return static_cast<double>(r >> 11) * (1.0 / 9007199254740992.0); }

// the halves of one pair added into 60 words
static void add_pair(const rg::Pair &p, int64_t sums[rg::kSumWords]) {
  int64_t term[rg::kTerms];
  rg::terms_of(p, term);
  for (int k = 0; k < rg::kTerms; ++k) {
    sums[2 * k] += rg::low_of(term[k]);
    sums[2 * k + 1] += rg::high_of(term[k]);
  }
}

int main(int argc, char **argv) {
  const int64_t count = argc > 1 ? std::strtoll(argv[1], nullptr, 10) : 1500;
  uint64_t bad = 0;
  auto fail = [&](const char *what, double a, double b) {
    if (bad < 10) std::fprintf(stderr, "mismatch (%s): %.17g %.17g\n", what, a, b);
    ++bad;
  };
  rg::Rule r;
  // RG3 / RG4 / RG7: the bounds
  if (rg::prepare(0.05f, 0.02f, 1, 20, 100, 1e-5, rg::kDefaultCondTol, &r)) fail("defaults refused", 0, 0);
  if (r.t != gn::threshold_of(0.05f) || r.tau2 != static_cast<int64_t>(std::floor(std::pow(static_cast<double>(0.02f) * 1048576.0, 2))))
    fail("rule", r.t, static_cast<double>(r.tau2));
  if (rg::prepare(0.005f, 0.005f, 1, 1, 1, 0.0, 1e-12, &r) || rg::prepare(0.5f, 0.5f, 7, 1000, 1, 1.0, 0.5, &r)) fail("bounds refused", 0, 0);
  if (!rg::prepare(std::nextafter(0.005f, 0.0f), 0.001f, 1, 20, 100, 1e-5, 1e-3, &r) || !rg::prepare(std::nextafter(0.5f, 1.0f), 0.02f, 1, 20, 100, 1e-5, 1e-3, &r) ||
      !rg::prepare(NAN, 0.02f, 1, 20, 100, 1e-5, 1e-3, &r))
    fail("match_radius taken", 0, 0);
  if (!rg::prepare(0.05f, 0.0f, 1, 20, 100, 1e-5, 1e-3, &r) || !rg::prepare(0.05f, std::nextafter(0.05f, 1.0f), 1, 20, 100, 1e-5, 1e-3, &r) ||
      !rg::prepare(0.05f, NAN, 1, 20, 100, 1e-5, 1e-3, &r))
    fail("max_plane_distance taken", 0, 0);
  if (!rg::prepare(0.05f, 0.02f, 0, 20, 100, 1e-5, 1e-3, &r) || !rg::prepare(0.05f, 0.02f, 1, 0, 100, 1e-5, 1e-3, &r) ||
      !rg::prepare(0.05f, 0.02f, 1, 1001, 100, 1e-5, 1e-3, &r) || !rg::prepare(0.05f, 0.02f, 1, 20, 0, 1e-5, 1e-3, &r))
    fail("stride / iterations / min_pairs taken", 0, 0);
  if (!rg::prepare(0.05f, 0.02f, 1, 20, 100, -1e-9, 1e-3, &r) || !rg::prepare(0.05f, 0.02f, 1, 20, 100, NAN, 1e-3, &r) ||
      !rg::prepare(0.05f, 0.02f, 1, 20, 100, 1e-5, 0.0, &r) || !rg::prepare(0.05f, 0.02f, 1, 20, 100, 1e-5, 1.0, &r) ||
      !rg::prepare(0.05f, 0.02f, 1, 20, 100, 1e-5, NAN, &r))
    fail("tolerance / cond_tol taken", 0, 0);

  // RG1: the identity, the fixed sequence against long double, the 4 x 4 and back
  {
    rg::Transform T;
    rg::set_identity(T);
    if (!rg::is_identity(T)) fail("identity", 0, 0);
    const double c[3] = {3.25, -1.5, 0.75};
    double M[16];
    rg::matrix_of(T, c, M);
    for (int a = 0; a < 16; ++a)
      if (M[a] != ((a % 5) == 0 ? 1.0 : 0.0)) fail("identity matrix", a, M[a]);
    rg::Transform back;
    if (!rg::from_matrix(M, c, &back) || !rg::is_identity(back)) fail("identity round trip", 0, 0);
    const double up[6] = {0.002, -0.003, 0.0015, 0.004, -0.001, 0.002};
    rg::compose(T, up);
    if (rg::is_identity(T)) fail("composed identity", 0, 0);
    const double len = std::sqrt(T.q[0] * T.q[0] + T.q[1] * T.q[1] + T.q[2] * T.q[2] + T.q[3] * T.q[3]);
    if (std::fabs(len - 1.0) > 4e-16) fail("unit quaternion", len, 1);
    rg::Frame f;
    rg::rotation_of(T.q, f.R);
    for (int a = 0; a < 3; ++a) f.c[a] = c[a], f.t[a] = T.t[a];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double dot = f.R[3 * a] * f.R[3 * b] + f.R[3 * a + 1] * f.R[3 * b + 1] + f.R[3 * a + 2] * f.R[3 * b + 2];
        if (std::fabs(dot - (a == b ? 1.0 : 0.0)) > 1e-15) fail("orthonormal", a, b);
      }
    // the rotation is that of the vector omega to second order: R x ~ x + omega x x
    if (std::fabs(f.R[1] + up[2]) > 1e-5 || std::fabs(f.R[2] - up[1]) > 1e-5 || std::fabs(f.R[5] + up[0]) > 1e-5) fail("sense of the rotation", f.R[1], up[2]);
    for (int64_t k = 0; k < count; ++k) {
      const float x = static_cast<float>(3.0 + unit(mix(3 * k))), y = static_cast<float>(-2.0 + unit(mix(3 * k + 1))),
                  z = static_cast<float>(1.0 + unit(mix(3 * k + 2)));
      float o[3];
      rg::apply(f, x, y, z, o);
      const long double d[3] = {static_cast<long double>(x) - c[0], static_cast<long double>(y) - c[1], static_cast<long double>(z) - c[2]};
      for (int a = 0; a < 3; ++a) {
        const long double want = f.R[3 * a] * d[0] + f.R[3 * a + 1] * d[1] + f.R[3 * a + 2] * d[2] + c[a] + f.t[a];
        if (std::fabs(static_cast<double>(want - o[a])) > 3e-7) fail("apply", o[a], static_cast<double>(want));
      }
    }
    rg::matrix_of(T, c, M);
    if (!rg::from_matrix(M, c, &back)) fail("round trip refused", 0, 0);
    for (int a = 0; a < 4; ++a)
      if (std::fabs(back.q[a] - T.q[a]) > 1e-15) fail("round trip q", back.q[a], T.q[a]);
    for (int a = 0; a < 3; ++a)
      if (std::fabs(back.t[a] - T.t[a]) > 1e-14) fail("round trip t", back.t[a], T.t[a]);
    // every branch of the conversion: half turns about the axes
    for (int axis = 0; axis < 3; ++axis) {
      double H[16] = {-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1};
      H[5 * axis] = 1.0;
      rg::Transform h;
      if (!rg::from_matrix(H, c, &h) || std::fabs(std::fabs(h.q[1 + axis]) - 1.0) > 1e-15 || std::fabs(h.q[0]) > 1e-15) fail("half turn", axis, h.q[0]);
    }
    M[0] += 1e-6;
    if (rg::from_matrix(M, c, &back)) fail("a sheared matrix taken", 0, 0);
    M[0] -= 1e-6;
    M[12] = 1e-3;
    if (rg::from_matrix(M, c, &back)) fail("a projective row taken", 0, 0);
    double mirror[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1};
    if (rg::from_matrix(mirror, c, &back)) fail("a mirror taken", 0, 0);
    mirror[10] = NAN;
    if (rg::from_matrix(mirror, c, &back)) fail("a NaN taken", 0, 0);
    const float mn[3] = {1.0f, 2.0f, 3.0f}, mx[3] = {2.0f, 4.0f, 7.0f};
    double pc[3], ell;
    rg::pivot_of(mn, mx, pc, &ell);
    if (pc[0] != 1.5 || pc[1] != 3.0 || pc[2] != 5.0 || ell != std::sqrt(21.0) * 0.5) fail("pivot", pc[0], ell);
    rg::pivot_of(mn, mn, pc, &ell);
    if (ell != 1.0) fail("a point's scale", ell, 1);
  }

  // RG3: the key orders by d2, then by the index; the threshold's two sides
  {
    const uint64_t a = rg::key_of(0.01f, 0.0f, 0.0f, 9), b = rg::key_of(0.0f, 0.01f, 0.0f, 4), c = rg::key_of(0.0f, 0.0f, std::nextafter(0.01f, 1.0f), 0);
    if (!(b < a && a < c)) fail("key order", 0, 0);
    if (rg::d2_of_key(a) != 0.01f * 0.01f || (a & 0xffffffffull) != 9) fail("key parts", rg::d2_of_key(a), 0);
    if (rg::key_of(0.0f, 0.0f, 0.0f, 5) != 5) fail("zero distance", 0, 0);
    if (rg::d2_of_key(~uint64_t(0)) <= 1e30f) fail("the empty key passes", 0, 0);
  }
  // MC1's test of the partner's normal
  {
    int32_t N[3];
    if (rg::normal_of(0.0f, 0.0f, 0.0f, N) || rg::normal_of(NAN, 0.0f, 1.0f, N) || rg::normal_of(0.0f, 1.5f, 0.0f, N) ||
        rg::normal_of(0.0002f, 0.0001f, 0.0f, N) || rg::normal_of(INFINITY, 0.0f, 0.0f, N))
      fail("an invalid normal taken", 0, 0);
    if (!rg::normal_of(0.6f, 0.0f, -0.8f, N) || N[0] != 1229 || N[1] != 0 || N[2] != -1638) fail("quanta of the normal", N[0], N[2]);
  }
  // RG4: the lever arm, ties to even, and its range
  {
    if (rg::lever_of(1024.00390625f, 0.0) != rg::kMaxLever + 1 || rg::lever_of(-1024.0f, 0.0) != -rg::kMaxLever || rg::lever_of(1.0f, 0.0) != 256 || rg::lever_of(0.5f / 256.0f, 0.0) != 0 || rg::lever_of(1.5f / 256.0f, 0.0) != 2 ||
        rg::lever_of(-2.5f / 256.0f, 0.0) != -2 || rg::lever_of(3.0f, 3.25) != -64)
      fail("lever_of", 0, 0);
    const double c[3] = {0.0, 0.0, 0.0};
    float mn[3] = {-1024.0f, -1.0f, -1.0f}, mx[3] = {1.0f, 1024.0f, 1.0f};
    if (!rg::levers_hold(mn, mx, c)) fail("the lever at 2^18 refused", 0, 0);
    mx[1] = 1024.00390625f;  // (2^18 + 1 quanta, exact in fp32)
    if (rg::levers_hold(mn, mx, c)) fail("the lever beyond 2^18 taken", 0, 0);
    mx[1] = 1.0f;
    mn[2] = -1024.00390625f;
    if (rg::levers_hold(mn, mx, c)) fail("the negative lever beyond 2^18 taken", 0, 0);
  }
  // RG4: the trim's boundary, normal (0, 0, 1), max_plane_distance a whole number of quanta
  {
    const float q = 1.0f / 1048576.0f;
    if (rg::prepare(0.05f, 2000.0f * q, 1, 20, 1, 1e-5, 1e-3, &r)) fail("trim rule", 0, 0);
    if (r.tau2 != 4000000) fail("tau2", static_cast<double>(r.tau2), 0);
    const int32_t N[3] = {0, 0, 2048};
    const int64_t u[3] = {256, -512, 7};
    rg::Pair p;
    if (!rg::pair_of(r.tau2, 100.0f * q, 0.0f, 2000.0f * q, N, u, p) || p.h != 2000 * 2048 || p.N2 != 4194304) fail("on the boundary", static_cast<double>(p.h), 0);
    if (p.g[0] != -512 * 2048 || p.g[1] != -256 * 2048 || p.g[2] != 0 || p.g[5] != 2048) fail("u x N", static_cast<double>(p.g[0]), static_cast<double>(p.g[1]));
    if (rg::pair_of(r.tau2, 0.0f, 0.0f, 2001.0f * q, N, u, p) || rg::pair_of(r.tau2, 0.0f, 0.0f, -2001.0f * q, N, u, p)) fail("one quantum beyond", 0, 0);
    if (!rg::pair_of(r.tau2, 0.0f, 0.0f, -2000.0f * q, N, u, p) || p.h != -2000 * 2048) fail("the other side", 0, 0);
  }

  // RG4 / RG5: the terms and their halves against 128-bit arithmetic, the widest ranges, the order of the pairs
  {
    if (rg::prepare(0.5f, 0.5f, 1, 20, 1, 1e-5, 1e-3, &r)) fail("widest rule", 0, 0);
    std::vector<rg::Pair> kept;
    __int128 want[rg::kTerms];
    for (int k = 0; k < rg::kTerms; ++k) want[k] = 0;
    for (int64_t k = 0; k < count; ++k) {
      float d[3];
      int32_t N[3];
      int64_t u[3];
      for (int a = 0; a < 3; ++a) {
        const uint64_t s = static_cast<uint64_t>(6 * k + a);
        d[a] = static_cast<float>((2.0 * unit(mix(100 + s)) - 1.0) * 0.5);
        N[a] = k == 0 ? 2048 : static_cast<int32_t>(std::lrint((2.0 * unit(mix(7000 + s)) - 1.0) * 2048.0));
        u[a] = k < 8 ? ((k >> a) & 1 ? rg::kMaxLever : -rg::kMaxLever) : static_cast<int64_t>(std::llrint((2.0 * unit(mix(90000 + s)) - 1.0) * 262144.0));
      }
      if (k < 8) d[0] = d[1] = d[2] = (k & 1) ? 0.28f : -0.28f;  // (d2 = 0.2352 <= 0.25: the rim of the widest sphere)
      if (!((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= r.t) || (N[0] == 0 && N[1] == 0 && N[2] == 0)) continue;
      if (!rg::terms_hold(r.tau2, d[0], d[1], d[2], N, u)) fail("ranges", d[0], static_cast<double>(u[0]));
      rg::Pair p;
      if (!rg::pair_of(r.tau2, d[0], d[1], d[2], N, u, p)) continue;
      kept.push_back(p);
      const __int128 g[6] = {p.g[0], p.g[1], p.g[2], p.g[3], p.g[4], p.g[5]}, h = p.h;
      int t = 0;
      for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) want[t++] += g[a] * g[b];
      for (int a = 0; a < 6; ++a) want[t++] += g[a] * h;
      want[t++] += h * h;
      want[t++] += p.N2;
      want[t++] += 1;
    }
    if (kept.size() < 16) fail("too few pairs kept", static_cast<double>(kept.size()), 0);
    int64_t fwd[rg::kSumWords] = {0}, bwd[rg::kSumWords] = {0};
    for (size_t k = 0; k < kept.size(); ++k) add_pair(kept[k], fwd);
    for (size_t k = kept.size(); k-- > 0;) add_pair(kept[k], bwd);
    if (std::memcmp(fwd, bwd, sizeof fwd) != 0) fail("order of the pairs", 0, 0);
    for (int k = 0; k < rg::kTerms; ++k) {
      const __int128 got = static_cast<__int128>(fwd[2 * k]) + static_cast<__int128>(fwd[2 * k + 1]) * 4294967296ll;
      if (got != want[k]) fail("sums", static_cast<double>(got), static_cast<double>(want[k]));
      if (fwd[2 * k] < 0) fail("a low half below zero", k, static_cast<double>(fwd[2 * k]));
    }
    if (rg::low_of(-1) != 0xffffffffll || rg::high_of(-1) != -1 || rg::low_of(int64_t(5) << 32) != 0 || rg::high_of(int64_t(5) << 32) != 5) fail("halves", 0, 0);
  }

  // RG6: a planted update is recovered at rank 6; on one plane the three unobservable components are exactly zero; rank 0
  {
    const double ell = 0.8, truth[6] = {0.001, -0.002, 0.0015, 0.003, -0.001, 0.002};
    for (int planes = 3; planes >= 0; planes -= (planes == 3 ? 2 : 1)) {  // 3 walls, 1 wall, none
      int64_t sums[rg::kSumWords] = {0};
      for (int64_t k = 0; k < (planes ? count : 0); ++k) {
        const int axis = static_cast<int>(k % planes == 0 ? 2 : k % planes - 1);  // (one wall: the normal is +z)
        int32_t N[3] = {0, 0, 0};
        N[axis] = 2048;
        double b[3];
        for (int a = 0; a < 3; ++a) b[a] = unit(mix(40 + 3 * static_cast<uint64_t>(k) + a)) - 0.5;
        b[axis] = 0.0;
        rg::Pair p;
        const int64_t u[3] = {std::llrint(b[0] * 256.0), std::llrint(b[1] * 256.0), std::llrint(b[2] * 256.0)};
        const double lever[3] = {u[0] / 256.0, u[1] / 256.0, u[2] / 256.0};
        // the residual the planted update leaves along the normal: n . (omega x b + dt), in offset quanta
        const double w[3] = {truth[1] * lever[2] - truth[2] * lever[1], truth[2] * lever[0] - truth[0] * lever[2], truth[0] * lever[1] - truth[1] * lever[0]};
        float d[3] = {0.0f, 0.0f, 0.0f};
        d[axis] = static_cast<float>(std::nearbyint((w[axis] + truth[3 + axis]) * 1048576.0) / 1048576.0);
        if (!rg::pair_of(int64_t(1) << 38, d[0], d[1], d[2], N, u, p)) fail("planted pair trimmed", 0, 0);
        add_pair(p, sums);
      }
      double up[6], eig[6];
      const int32_t dof = rg::solve(sums, ell, 1e-6, up, eig);
      if (dof != (planes == 3 ? 6 : planes == 1 ? 3 : 0)) fail("dof", dof, planes);
      for (int a = 0; a < 6; ++a) {
        const bool seen = planes == 3 || (planes == 1 && (a == 0 || a == 1 || a == 5));
        if (seen && std::fabs(up[a] - truth[a]) > 2e-6) fail("planted update", up[a], truth[a]);
        if (!seen && up[a] != 0.0) fail("an unobservable component moved", a, up[a]);
      }
      if (planes == 0 && rg::rms_of(sums) != 0.0) fail("rms without pairs", 0, 0);
    }
    // a sum that needs both halves: 2^31 - 64 pairs' worth of the largest g_0 g_0, folded as the kernel's reduce would
    int64_t big[rg::kSumWords] = {0};
    const __int128 term = static_cast<__int128>(1) << 60, pairs = (static_cast<__int128>(1) << 31) - 64, total = term * pairs;
    big[0] = static_cast<int64_t>((term & 0xffffffff) * pairs);
    big[1] = static_cast<int64_t>((term >> 32) * pairs);
    if (total <= (static_cast<__int128>(1) << 63)) fail("the sum fits one word", 0, 0);
    if (rg::sum_of(big, 0) != static_cast<double>(total)) fail("both halves", rg::sum_of(big, 0), static_cast<double>(total));
    big[0] = int64_t(0xffffffffll) * 2147483584ll;  // (the low halves at their largest)
    const double both = static_cast<double>(total + static_cast<__int128>(big[0]));  // (two roundings against one: an ulp)
    if (std::fabs(rg::sum_of(big, 0) - both) > both * 2.3e-16) fail("the low half's range", rg::sum_of(big, 0), both);
  }

  // RG7: the loop's three endings, with an evaluation that is told what to answer
  {
    if (rg::prepare(0.05f, 0.02f, 1, 4, 10, 1e-5, 1e-3, &r)) fail("loop rule", 0, 0);
    rg::Transform T;
    int64_t sums[rg::kSumWords];
    double log[4 * rg::kLogWords];
    int32_t st[2];
    auto few = [&](const rg::Transform &, int64_t *out) {
      for (int a = 0; a < rg::kSumWords; ++a) out[a] = 0;
      out[58] = 9;
      return 0;
    };
    rg::set_identity(T);
    if (rg::iterate(r, 1.0, T, few, sums, log, st) != 0 || st[0] != rg::kTooFewPairs || st[1] != 1 || !rg::is_identity(T) || log[0] != 9.0) fail("too few pairs", st[0], st[1]);
    auto still = [&](const rg::Transform &, int64_t *out) {  // pairs on three walls with no residual: a zero update
      for (int a = 0; a < rg::kSumWords; ++a) out[a] = 0;
      for (int axis = 0; axis < 3; ++axis)
        for (int k = 0; k < 20; ++k) {
          int32_t N[3] = {0, 0, 0};
          N[axis] = 2048;
          const int64_t u[3] = {static_cast<int64_t>(mix(3 * k) % 257) - 128, static_cast<int64_t>(mix(3 * k + 1) % 257) - 128, static_cast<int64_t>(mix(3 * k + 2) % 257) - 128};
          rg::Pair p;
          rg::pair_of(1, 0.0f, 0.0f, 0.0f, N, u, p);
          add_pair(p, out);
        }
      return 0;
    };
    if (rg::iterate(r, 1.0, T, still, sums, log, st) != 0 || st[0] != rg::kConverged || st[1] != 1 || log[2] != 6.0 || log[3] != 0.0) fail("converged", st[0], log[2]);
    int calls = 0;
    auto drifting = [&](const rg::Transform &, int64_t *out) {  // the same residual every time: never below the tolerance
      ++calls;
      for (int a = 0; a < rg::kSumWords; ++a) out[a] = 0;
      for (int axis = 0; axis < 3; ++axis)
        for (int k = 0; k < 20; ++k) {
          int32_t N[3] = {0, 0, 0};
          N[axis] = 2048;
          const int64_t u[3] = {static_cast<int64_t>(mix(3 * k) % 257) - 128, static_cast<int64_t>(mix(3 * k + 1) % 257) - 128, static_cast<int64_t>(mix(3 * k + 2) % 257) - 128};
          float d[3] = {0.0f, 0.0f, 0.0f};
          d[axis] = 0.001f;
          rg::Pair p;
          rg::pair_of(int64_t(1) << 38, d[0], d[1], d[2], N, u, p);
          add_pair(p, out);
        }
      return 0;
    };
    rg::set_identity(T);
    if (rg::iterate(r, 1.0, T, drifting, sums, log, st) != 0 || st[0] != rg::kIterationLimit || st[1] != 4 || calls != 4) fail("iteration limit", st[0], calls);
    if (std::fabs(T.t[0] - 0.004) > 1e-5 || std::fabs(log[3 * rg::kLogWords + 4] - 0.001 * std::sqrt(3.0)) > 1e-5) fail("four steps of 1 mm", T.t[0], log[19]);
    auto broken = [&](const rg::Transform &, int64_t *) { return -5; };
    if (rg::iterate(r, 1.0, T, broken, sums, log, st) != -5) fail("an error is passed on", 0, 0);
  }
  std::printf("%llu mismatches\n", static_cast<unsigned long long>(bad));
  return bad ? 1 : 0;
}
