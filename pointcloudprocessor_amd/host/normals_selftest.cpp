// normals_selftest -- csrc/pcp_normals.hpp compiled for the host (CPU only: never a GPU job; meant to be built with
// -fsanitize=address,undefined as well).  Checks the threshold rule, the quantisation (exact product, ties to even, the bound
// on |q|), the moments of a random cloud against sums taken in 128-bit integers and their invariance under the order of the
// candidates, and the covariance against the same three operations written out.  Prints the number of mismatches; exit code 0
// iff none.   usage: normals_selftest [points]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/pcp_normals.hpp"

using namespace pcp;

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

static float unit(uint64_t r) { return static_cast<float>(static_cast<double>(r >> 11) * (1.0 / 9007199254740992.0)); }

int main(int argc, char **argv) {
  const int64_t count = argc > 1 ? std::strtoll(argv[1], nullptr, 10) : 1500;
  uint64_t bad = 0;
  auto fail = [&](const char *what, double a, double b) {
    if (bad < 10) std::fprintf(stderr, "mismatch (%s): %.17g %.17g\n", what, a, b);
    ++bad;
  };
  if (!gn::radius_ok(0.005f) || !gn::radius_ok(1.0f) || gn::radius_ok(0.0049f) || gn::radius_ok(1.0001f) || gn::radius_ok(NAN) ||
      gn::radius_ok(-0.1f) || gn::radius_ok(INFINITY))
    fail("radius_ok", 0, 0);
  const float radii[] = {0.005f, 0.03f, 0.1f, 0.3f, 0.5f, 0.7f, 1.0f};
  for (float r : radii) {  // t is the largest float not above r^2
    const float t = gn::threshold_of(r);
    const double r2 = static_cast<double>(r) * static_cast<double>(r);
    if (!(static_cast<double>(t) <= r2) || !(static_cast<double>(std::nextafter(t, 2.0f)) > r2)) fail("threshold_of", t, r2);
  }
  // quantisation: ties to even, exact product, the bound
  if (gn::quantise(0.5f / 1048576.0f) != 0 || gn::quantise(1.5f / 1048576.0f) != 2 || gn::quantise(-2.5f / 1048576.0f) != -2 ||
      gn::quantise(1.0f) != 1048576 || gn::quantise(-1.0f) != -1048576 || gn::quantise(0.0f) != 0 || gn::quantise(-0.0f) != 0)
    fail("quantise", 0, 0);
  for (int64_t k = 0; k < count * 100; ++k) {
    const float d = (2.0f * unit(mix(static_cast<uint64_t>(k))) - 1.0f) * 1.0000001f;
    const int32_t q = gn::quantise(d);
    const double exact = static_cast<double>(d) * 1048576.0;
    if (std::fabs(static_cast<double>(q) - exact) > 0.5 || q > gn::kMaxQuantum || q < -gn::kMaxQuantum) fail("quantise range", q, exact);
    if (q != static_cast<int32_t>(std::nearbyint(exact))) fail("quantise rint", q, exact);
  }
  if (!gn::finite3(0.0f, -1.0f, 3.4e38f) || gn::finite3(NAN, 0.0f, 0.0f) || gn::finite3(0.0f, INFINITY, 0.0f) || gn::finite3(0.0f, 0.0f, -INFINITY))
    fail("finite3", 0, 0);
  // moments of a random cloud in a 2 m cube with duplicates, against 128-bit sums; forwards and backwards
  const int64_t n = count;
  std::vector<float> p(static_cast<size_t>(3 * n));
  for (int64_t i = 0; i < 3 * n; ++i) p[static_cast<size_t>(i)] = 8.0f + 2.0f * unit(mix(0xabcdefull + static_cast<uint64_t>(i)));
  for (int64_t i = 0; i + 7 < n; i += 7)
    for (int a = 0; a < 3; ++a) p[static_cast<size_t>(3 * (i + 3) + a)] = p[static_cast<size_t>(3 * i + a)];  // exact duplicates
  for (float r : {0.3f, 1.0f}) {
    const float t = gn::threshold_of(r);
    for (int64_t i = 0; i < n; ++i) {
      const float *q = &p[static_cast<size_t>(3 * i)];
      gn::Moments fwd, bwd;
      gn::clear(fwd);
      gn::clear(bwd);
      __int128 s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int64_t j = 0; j < n; ++j) {
        const float *c = &p[static_cast<size_t>(3 * j)];
        const float dx = c[0] - q[0], dy = c[1] - q[1], dz = c[2] - q[2];
        const bool in = gn::visit(fwd, dx, dy, dz, t);
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (in != (static_cast<double>(d2) <= static_cast<double>(r) * static_cast<double>(r))) fail("neighbour rule", d2, r);
        if (in) {
          const __int128 x = gn::quantise(dx), y = gn::quantise(dy), z = gn::quantise(dz);
          const __int128 add[10] = {1, x, y, z, x * x, x * y, x * z, y * y, y * z, z * z};
          for (int a = 0; a < 10; ++a) s[a] += add[a];
        }
      }
      for (int64_t j = n - 1; j >= 0; --j) {
        const float *c = &p[static_cast<size_t>(3 * j)];
        gn::visit(bwd, c[0] - q[0], c[1] - q[1], c[2] - q[2], t);
      }
      int64_t a_[10], b_[10];
      gn::store(fwd, a_);
      gn::store(bwd, b_);
      if (std::memcmp(a_, b_, sizeof(a_)) != 0) fail("order of the candidates", static_cast<double>(i), r);
      for (int a = 0; a < 10; ++a)
        if (static_cast<__int128>(a_[a]) != s[a]) fail("moments", static_cast<double>(a_[a]), static_cast<double>(s[a]));
      if (fwd.n < 1) fail("a point is its own neighbour", static_cast<double>(i), 0);
      double C[6];
      gn::covariance(fwd, C);
      const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
      for (int e = 0; e < 6; ++e) {
        const volatile double prod = static_cast<double>(fwd.s1[ia[e]]) * static_cast<double>(fwd.s1[ib[e]]);
        const volatile double quo = prod / static_cast<double>(fwd.n);
        const double want = static_cast<double>(fwd.s2[e]) - quo;
        if (std::memcmp(&want, &C[e], 8) != 0) fail("covariance", want, C[e]);
      }
    }
  }
  std::printf("%llu mismatches\n", static_cast<unsigned long long>(bad));
  return bad ? 1 : 0;
}
