// pcp_compare.hpp -- the rule of the map comparison ("Map comparison", MC1-MC6), one copy for the kernel
// (pcp_compare.hip), the CPU form (pcp_compare_host) and the host self-test (host/compare_selftest.cpp).  Per core point of
// the map, the points of the map (epoch A) and of the base (epoch B) inside a cylinder along the point's oriented normal are
// summed in exact 64-bit integers (offsets quantised to 2^-20 m as in pcp_normals.hpp, the normal to 2^-11), so the sums are a
// function of the SET of candidates: no dependence on their order, the grid, the cell size or the input order.  The finish
// is a fixed sequence of fp64 operations.  Build without floating-point contraction: every fp32 / fp64 operation below is
// rounded on its own.
//
// Ranges (MC3).  search_radius <= 0.5, so an offset that passes the sphere test has fl32(d2) <= t <= 0.25: every |d_a| <=
// 0.5 (1 + 2^-23), |q_a| <= 2^19 + 1, and Q2 = q.q <= 2^38 (1 + 2^-17) (the rounding of d2 and the three roundings to the
// quantum move Q2 by less than 2^-17 of itself).  A valid normal has every |n_a| <= 1, so |N_a| <= 2^11 and N2 = N.N <=
// 3 * 2^22; a unit normal has N2 <= 2^22 (1 + 2^-9).  By Cauchy-Schwarz h^2 <= Q2 * N2, so with a unit normal |h| <
// 2^30 (1 + 2^-9) < 2^31, h^2 < 2^62, Q2 * N2 <= 2^60 (1 + 2^-8) and, with rc2, L2 <= 2^38 (rc, L < search_radius <= 0.5),
// rc2 * N2, L2 * N2 <= 2^60 (1 + 2^-9).  With the longest normal the rule admits (N2 = 3 * 2^22) the same products are
// bounded by 3 * 2^60 (1 + 2^-17) < 2^62 and |h| < 1.74 * 2^30 < 2^31.  Q2 * N2 - h^2 lies in [0, Q2 * N2].  Every product
// fits a signed 64-bit word; bounds_hold() re-derives it in 128-bit arithmetic and the host form asserts it per candidate.
// Sums (MC4): fewer than 2^22 candidates per epoch, so |S1| < 2^53, S2a < 2^54, S2b < 2^52: no carries.
#pragma once

#include <cmath>
#include <cstdint>

#include "pcp_normals.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCP_MC_HD __host__ __device__ __forceinline__
#else
#define PCP_MC_HD inline
#endif

namespace pcp {
namespace mc {

constexpr float kNormalScale = 2048.0f;                // MC2: 2^11 quanta per unit of the normal
constexpr int64_t kMaxCandidates = int64_t(1) << 22;   // MC4: an epoch with this many candidates at one point is PCP_ERR_RANGE
constexpr int kSumWords = 8;                           // nA S1A S2aA S2bA nB S1B S2aB S2bB
constexpr float kMinExtent = 0.005f, kMaxSearch = 0.5f;  // MC3's bounds

enum Status : uint8_t { kNotCore = 0, kNoCounterpart = 1, kTooFewOwn = 2, kMeasured = 3, kPositive = 4, kNegative = 5 };

// what a call fixes for every point
struct Rule {
  float search_radius, t;  // MC3's sphere
  int64_t rc2, L2;         // MC3's cylinder, in squared offset quanta
  int32_t min_points, orient_mode;
  float orient[3];
  double reg_error;
};

// MC3 / MC6: the parameters' bounds; nullptr, or what is wrong.  NaN fails every test.
inline const char *prepare(float rc, float L, float reg_error, int32_t min_points, int32_t orient_mode, const float orient[3],
                           Rule *out) {
  if (!(rc >= kMinExtent)) return "cyl_radius below 0.005 (or not finite)";
  if (!(L >= kMinExtent)) return "cyl_half_length below 0.005 (or not finite)";
  const double drc = static_cast<double>(rc), dl = static_cast<double>(L);
  const float s = std::nextafter(static_cast<float>(std::sqrt(drc * drc + dl * dl)), INFINITY);
  if (!(s <= kMaxSearch)) return "search radius sqrt(cyl_radius^2 + cyl_half_length^2) above 0.5";
  if (!(reg_error >= 0.0f) || !(reg_error <= 3.402823466e+38f)) return "reg_error negative or not finite";
  if (min_points < 2) return "min_points below 2";
  if (orient_mode < 0 || orient_mode > 2) return "orient_mode outside 0..2";
  if (orient_mode != 0 && !gn::finite3(orient[0], orient[1], orient[2])) return "orient not finite";
  Rule r{};
  r.search_radius = s;
  r.t = gn::threshold_of(s);
  const double qrc = drc * 1048576.0, ql = dl * 1048576.0;  // (exact: a power of two)
  r.rc2 = static_cast<int64_t>(std::floor(qrc * qrc));       // (exact: 48 bits at most)
  r.L2 = static_cast<int64_t>(std::floor(ql * ql));
  r.min_points = min_points;
  r.orient_mode = orient_mode;
  for (int a = 0; a < 3; ++a) r.orient[a] = orient_mode != 0 ? orient[a] : 0.0f;
  r.reg_error = static_cast<double>(reg_error);
  *out = r;
  return nullptr;
}

// MC2's rounding of one component: rint(n_a * 2^11), ties to even (the product is exact: a power of two, |n_a| <= 1)
PCP_MC_HD int32_t quantise_normal(float v) {
  const float p = v * kNormalScale;
#if defined(__HIP_DEVICE_COMPILE__)
  return __float2int_rn(p);
#else
  return static_cast<int32_t>(lrintf(p));
#endif
}

// the oriented integer direction of one core point and what depends on it alone
struct Direction {
  int32_t N[3];
  int64_t N2, rc2N2, L2N2;
};

// MC1 / MC2 for the finite point p with the fp32 normal n: false = not a core point (status 0)
PCP_MC_HD bool direction(const Rule &r, float px, float py, float pz, float nx, float ny, float nz, Direction &d) {
  if (!gn::finite3(nx, ny, nz)) return false;
  if (!(fabsf(nx) <= 1.0f && fabsf(ny) <= 1.0f && fabsf(nz) <= 1.0f)) return false;
  if (nx == 0.0f && ny == 0.0f && nz == 0.0f) return false;
  if (r.orient_mode != 0) {
    float vx = r.orient[0], vy = r.orient[1], vz = r.orient[2];
    if (r.orient_mode == 1) {
      vx = vx - px;
      vy = vy - py;
      vz = vz - pz;
    }
    const float dot = (nx * vx + ny * vy) + nz * vz;
    if (dot < 0.0f) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
  }
  d.N[0] = quantise_normal(nx);
  d.N[1] = quantise_normal(ny);
  d.N[2] = quantise_normal(nz);
  d.N2 = (static_cast<int64_t>(d.N[0]) * d.N[0] + static_cast<int64_t>(d.N[1]) * d.N[1]) + static_cast<int64_t>(d.N[2]) * d.N[2];
  d.rc2N2 = r.rc2 * d.N2;
  d.L2N2 = r.L2 * d.N2;
  return d.N2 != 0;
}

// MC4: the sums of one core point, the epochs under their own names (the kernel keeps them in registers)
struct Sums {
  int64_t nA, s1A, s2aA, s2bA;
  int64_t nB, s1B, s2aB, s2bB;
};

PCP_MC_HD void clear(Sums &s) { s.nA = s.s1A = s.s2aA = s.s2bA = s.nB = s.s1B = s.s2aB = s.s2bB = 0; }

// MC3's integer part for the quantised offset q: true iff inside the cylinder; h = q.N
PCP_MC_HD bool in_cylinder(const Direction &d, int32_t qx, int32_t qy, int32_t qz, int64_t &h) {
  h = (static_cast<int64_t>(qx) * d.N[0] + static_cast<int64_t>(qy) * d.N[1]) + static_cast<int64_t>(qz) * d.N[2];
  const int64_t Q2 = (static_cast<int64_t>(qx) * qx + static_cast<int64_t>(qy) * qy) + static_cast<int64_t>(qz) * qz;
  const int64_t hh = h * h;
  if (hh > d.L2N2) return false;
  return Q2 * d.N2 - hh <= d.rc2N2;
}

// MC3 + MC4 for one candidate of epoch `epoch` (0 = map, 1 = base) at offset d = candidate - query: the fp32 sphere test
// first, then the integer tests and the adds; true iff it was a candidate
PCP_MC_HD bool visit(Sums &s, const Direction &d, float t, float dx, float dy, float dz, uint32_t epoch) {
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  if (!(d2 <= t)) return false;
  int64_t h;
  if (!in_cylinder(d, gn::quantise(dx), gn::quantise(dy), gn::quantise(dz), h)) return false;
  const uint64_t hh = static_cast<uint64_t>(h * h);
  const int64_t lo = static_cast<int64_t>(hh & 0xffffffffull), hi = static_cast<int64_t>(hh >> 32);
  // both epochs' words are written, one side masked to zero: a branch on the epoch would let the compiler address the sums
  // through memory (scratch on the device)
  const int64_t mB = -static_cast<int64_t>(epoch & 1u), mA = ~mB;
  s.nA += 1 & mA;
  s.s1A += h & mA;
  s.s2aA += lo & mA;
  s.s2bA += hi & mA;
  s.nB += 1 & mB;
  s.s1B += h & mB;
  s.s2aB += lo & mB;
  s.s2bB += hi & mB;
  return true;
}

// The ranges of the header comment for one offset that passed the sphere test, re-derived in 128-bit arithmetic: every
// product of in_cylinder and of visit fits a signed 64-bit word and |h| < 2^31.  (Host only.)
inline bool bounds_hold(const Rule &r, const Direction &d, int32_t qx, int32_t qy, int32_t qz) {
  typedef __int128 wide;
  const wide lim62 = static_cast<wide>(1) << 62;
  const wide h = (static_cast<wide>(qx) * d.N[0] + static_cast<wide>(qy) * d.N[1]) + static_cast<wide>(qz) * d.N[2];
  const wide Q2 = (static_cast<wide>(qx) * qx + static_cast<wide>(qy) * qy) + static_cast<wide>(qz) * qz;
  const wide N2 = d.N2;
  const wide lim31 = static_cast<wide>(1) << 31;
  return h > -lim31 && h < lim31 && h * h < lim62 && Q2 * N2 < lim62 && static_cast<wide>(r.rc2) * N2 < lim62 &&
         static_cast<wide>(r.L2) * N2 < lim62 && Q2 * N2 - h * h >= 0;
}

struct Result {
  float distance, lod;
  uint8_t status;
};

// MC5's variance of one epoch (n >= 2); a rounding that leaves it below zero gives 0
PCP_MC_HD double variance(int64_t n, int64_t s1, int64_t s2a, int64_t s2b) {
  const double dn = static_cast<double>(n), d1 = static_cast<double>(s1);
  const double S2 = static_cast<double>(s2a) + 4294967296.0 * static_cast<double>(s2b);
  const double var = (S2 - (d1 * d1) / dn) / (dn - 1.0);
  return var > 0.0 ? var : 0.0;
}

// MC5 + MC6 for a core point
PCP_MC_HD Result finish(const Rule &r, const Direction &d, const Sums &s) {
  Result out;
  out.distance = 0.0f;
  out.lod = 0.0f;
  if (s.nB < r.min_points) {
    out.status = kNoCounterpart;
    return out;
  }
  if (s.nA < r.min_points) {
    out.status = kTooFewOwn;
    return out;
  }
  const double nA = static_cast<double>(s.nA), nB = static_cast<double>(s.nB);
  const double scale = sqrt(static_cast<double>(d.N2)) * 1048576.0;
  const double distance = (static_cast<double>(s.s1A) / nA - static_cast<double>(s.s1B) / nB) / scale;
  const double varA = variance(s.nA, s.s1A, s.s2aA, s.s2bA), varB = variance(s.nB, s.s1B, s.s2aB, s.s2bB);
  const double lod = 1.96 * sqrt(varA / nA + varB / nB) / scale + r.reg_error;
  out.status = fabs(distance) > lod ? (distance > 0.0 ? kPositive : kNegative) : kMeasured;
  out.distance = static_cast<float>(distance);
  out.lod = static_cast<float>(lod);
  return out;
}

PCP_MC_HD void store(const Sums &s, int64_t out[kSumWords]) {
  out[0] = s.nA, out[1] = s.s1A, out[2] = s.s2aA, out[3] = s.s2bA;
  out[4] = s.nB, out[5] = s.s1B, out[6] = s.s2aB, out[7] = s.s2bB;
}

}  // namespace mc
}  // namespace pcp
