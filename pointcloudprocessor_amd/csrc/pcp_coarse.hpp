// pcp_coarse.hpp -- the rule of the coarse registration ("Coarse registration", CG1-CG9), one copy for the kernels
// (pcp_coarse.hip), the CPU forms (pcp_coarse_*_host, pcp_compare_register_coarse_host) and the host self-test
// (host/coarse_selftest.cpp).  The base survey is brought near the map from an arbitrary pose: per keypoint an unsigned spin
// image of 8 x 8 integer bins about its quantised normal, matched by exact L1 distance, three correspondences per hypothesis
// drawn by a counter-based integer generator, every hypothesis scored by an exact integer inlier count, the winner refitted by
// Horn's quaternion solution over exact integer sums.  Counts and choices are integers; a pose is one fixed sequence of fp64
// operations.  Build without floating-point contraction: every fp32 / fp64 operation below is rounded on its own.
//
// Ranges (CG2).  support_radius <= 0.25, so an offset that passes the sphere test has every |q_a| <= 2^18 + 1 and Q2 = q.q <=
// 3 (2^18 + 1)^2 < 3 * 2^36 (1 + 2^-16); a valid normal has N2 <= 3 * 2^22, so Q2 * N2 <= 9 * 2^58 (1 + 2^-16) < 2^62 and, by
// Cauchy-Schwarz, h^2 <= Q2 * N2: W = Q2 * N2 - h^2 lies in [0, Q2 * N2].  E <= 2^18, so e_k^2 * N2 <= 2^36 * 3 * 2^22 < 2^60.
// bins_hold() re-derives it per pair in 128-bit arithmetic and the host form asserts it.
// Ranges (CG5).  An offset with a component above 1 m is no inlier before it is quantised (inlier_distance <= 0.5), so
// |q_a| <= 2^20 and Q2 <= 3 * 2^40.
// Ranges (CG6).  The refit's quanta are 2^-16 m about the two pivots, |u_a|, |v_a| <= 2^26 (1024 m), at most 2^18 inliers:
// |sum u_a v_b| <= 2^70, n times that <= 2^88: 128-bit integers on the host, Python's in the restatement.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "pcp_register.hpp"

namespace pcp {
namespace cg {

constexpr int kBins = 8;                                // CG2: radial x height
constexpr int kDescWords = kBins * kBins;               // uint16 per keypoint
constexpr int64_t kMaxKeypoints = int64_t(1) << 18;     // CG3: per side
constexpr int64_t kMaxCorrespondences = int64_t(1) << 18;
constexpr int32_t kMaxHypotheses = 1 << 16;             // CG4
constexpr int kSweeps = 12;                             // CG6: cyclic Jacobi sweeps over the 6 pairs (p < q, row by row)
constexpr double kRefitScale = 65536.0;                 // CG6: the refit's quantum is 2^-16 m
constexpr int64_t kMaxRefit = int64_t(1) << 26;
constexpr double kRunnerTrace = 2.969615506024416;      // CG6: 1 + 2 cos(10 deg): a rotation further than that has a smaller trace
constexpr int kReportWords = 16;                        // CG8
constexpr uint64_t kNoKey = ~uint64_t(0);

enum Status : int32_t { kFound = 0, kTooFewInliers = 2 };
enum Refusal : int32_t { kAccepted = 0, kRepeat = 1, kShortSide = 2, kSideMismatch = 3, kThin = 4 };
// CG8: the words of the report
enum Report : int { kKeyMap = 0, kKeyBase, kValidMap, kValidBase, kCorrespondences, kScored, kRefused, kWinner, kRunnerUp, kRefit, kKept,
                    kStatus, kWinnerH, kTriple0, kTriple1, kTriple2 };

// what a call fixes
struct Rule {
  float support_radius, t, normal_radius;
  int64_t edge2[kBins];  // CG2: e_k^2
  int32_t map_stride, base_stride, min_neighbours, min_offplane_permille, ratio_q8, mutual, hypotheses, min_inliers;
  uint64_t seed;
  int64_t tau2;  // CG5's bound, in squared offset quanta
  double min_side, side_tolerance, min_sin2;
};

// CG9: the parameters' bounds; nullptr, or what is wrong.  NaN fails every test.  P: pcp_coarse_params.
template <class P>
inline const char *prepare(const P &p, Rule *out) {
  if (!(p.support_radius >= 0.02f) || !(p.support_radius <= 0.25f)) return "support_radius outside 0.02..0.25 (or not finite)";
  if (!gn::radius_ok(p.normal_radius)) return "normal_radius outside 0.005..1 (or not finite)";
  if (!(p.inlier_distance >= mc::kMinExtent) || !(p.inlier_distance <= mc::kMaxSearch)) return "inlier_distance outside 0.005..0.5 (or not finite)";
  if (!(p.min_side > 0.0f) || !(p.min_side <= 1.0e6f)) return "min_side outside (0, 1e6]";
  if (!(p.side_tolerance >= 0.0f) || !(p.side_tolerance <= 1.0e6f)) return "side_tolerance outside 0..1e6";
  if (!(p.min_angle_deg > 0.0f) || !(p.min_angle_deg <= 60.0f)) return "min_angle_deg outside (0, 60]";
  if (p.map_stride < 1 || p.base_stride < 1) return "a stride below 1";
  if (p.min_neighbours < 1) return "min_neighbours below 1";
  if (p.min_offplane_permille < 0 || p.min_offplane_permille > 1000) return "min_offplane_permille outside 0..1000";
  if (p.ratio_q8 < 0 || p.ratio_q8 > 256) return "ratio_q8 outside 0..256";
  if (p.mutual != 0 && p.mutual != 1) return "mutual neither 0 nor 1";
  if (p.hypotheses < 1 || p.hypotheses > kMaxHypotheses) return "hypotheses outside 1..65536";
  if (p.min_inliers < 3) return "min_inliers below 3";
  Rule r{};
  r.support_radius = p.support_radius;
  r.t = gn::threshold_of(p.support_radius);
  r.normal_radius = p.normal_radius;
  const int64_t E = static_cast<int64_t>(std::rint(static_cast<double>(p.support_radius) * 1048576.0));  // (the product is exact)
  for (int k = 0; k < kBins; ++k) {
    const int64_t e = (k * E) / kBins;
    r.edge2[k] = e * e;
  }
  r.map_stride = p.map_stride, r.base_stride = p.base_stride;
  r.min_neighbours = p.min_neighbours, r.min_offplane_permille = p.min_offplane_permille;
  r.ratio_q8 = p.ratio_q8, r.mutual = p.mutual, r.hypotheses = p.hypotheses, r.min_inliers = p.min_inliers;
  r.seed = p.seed;
  const double qd = static_cast<double>(p.inlier_distance) * 1048576.0;
  r.tau2 = static_cast<int64_t>(std::floor(qd * qd));
  r.min_side = static_cast<double>(p.min_side);
  r.side_tolerance = static_cast<double>(p.side_tolerance);
  const double s = std::sin(static_cast<double>(p.min_angle_deg) * 0.017453292519943295);
  r.min_sin2 = s * s;
  *out = r;
  return nullptr;
}

// ---- CG2: the descriptor ---------------------------------------------------------------------------------------------------
// the axis of one keypoint and what depends on it alone: lim[k - 1] = e_k^2 * N2, k = 1 .. 7 (e_0 = 0 holds for every pair)
struct Axis {
  int64_t N[3], N2, lim[kBins - 1];
};

PCP_RG_HD void axis_of(const int64_t edge2[kBins], const int32_t N[3], Axis &a) {
  a.N[0] = N[0], a.N[1] = N[1], a.N[2] = N[2];
  a.N2 = (a.N[0] * a.N[0] + a.N[1] * a.N[1]) + a.N[2] * a.N[2];
PCP_RG_UNROLL
  for (int k = 1; k < kBins; ++k) a.lim[k - 1] = edge2[k] * a.N2;
}

// the bin (radial * 8 + height) of the point at offset d = point - keypoint, or -1 when it is no neighbour (fl32 d2 > t)
PCP_RG_HD int bin_of(const Axis &a, float t, float dx, float dy, float dz) {
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  if (!(d2 <= t)) return -1;
  const int64_t qx = gn::quantise(dx), qy = gn::quantise(dy), qz = gn::quantise(dz);
  const int64_t h = (qx * a.N[0] + qy * a.N[1]) + qz * a.N[2];
  const int64_t Q2 = (qx * qx + qy * qy) + qz * qz;
  const int64_t hh = h * h, W = Q2 * a.N2 - hh;
  int radial = 0, height = 0;
PCP_RG_UNROLL
  for (int k = 0; k < kBins - 1; ++k) {
    radial += a.lim[k] <= W ? 1 : 0;
    height += a.lim[k] <= hh ? 1 : 0;
  }
  return radial * kBins + height;
}

// n: the counts' total; plane: the total of the bins of height 0
PCP_RG_HD bool descriptor_ok(int32_t min_neighbours, int32_t min_offplane_permille, uint32_t n, uint32_t plane) {
  return n >= static_cast<uint32_t>(min_neighbours) &&
         static_cast<int64_t>(n - plane) * 1000 >= static_cast<int64_t>(min_offplane_permille) * static_cast<int64_t>(n);
}

PCP_RG_HD uint16_t scaled(uint32_t count, uint32_t n) {
  return static_cast<uint16_t>((static_cast<uint64_t>(count) * 65535u) / static_cast<uint64_t>(n));
}

// The ranges of the header comment for one pair that passed the sphere test, in 128-bit arithmetic.  (Host only.)
inline bool bins_hold(const Axis &a, float dx, float dy, float dz) {
  typedef __int128 wide;
  const wide lim62 = static_cast<wide>(1) << 62;
  const wide q[3] = {gn::quantise(dx), gn::quantise(dy), gn::quantise(dz)};
  const wide h = (q[0] * a.N[0] + q[1] * a.N[1]) + q[2] * a.N[2], Q2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
  const wide N2 = a.N2;
  return Q2 * N2 < lim62 && h * h < lim62 && Q2 * N2 - h * h >= 0 && static_cast<wide>(a.lim[kBins - 2]) < lim62;
}

// ---- CG3: matching ---------------------------------------------------------------------------------------------------------
PCP_RG_HD uint32_t l1_of(const uint16_t *a, const uint16_t *b) {
  uint32_t s = 0;
  for (int k = 0; k < kDescWords; ++k) s += a[k] > b[k] ? static_cast<uint32_t>(a[k] - b[k]) : static_cast<uint32_t>(b[k] - a[k]);
  return s;
}

// the two least keys (L1 << 32 | ordinal) seen; kNoKey = none
struct Best {
  uint64_t best, second;
};

PCP_RG_HD void offer(Best &b, uint64_t key) {
  const bool first = key < b.best, next = key < b.second;
  b.second = first ? b.best : (next ? key : b.second);
  b.best = first ? key : b.best;
}

// CG3's list: (base ordinal, map ordinal) in ascending base ordinal.  (Host only.)
inline void correspondences(const Rule &r, int64_t kb, const Best *base, const Best *map, std::vector<int32_t> &pairs) {
  pairs.clear();
  for (int64_t b = 0; b < kb; ++b) {
    if (base[b].best == kNoKey) continue;
    const uint64_t l1 = base[b].best >> 32, m = base[b].best & 0xffffffffull;
    if (base[b].second != kNoKey && !(l1 * 256u <= static_cast<uint64_t>(r.ratio_q8) * (base[b].second >> 32))) continue;
    if (r.mutual && (map[m].best & 0xffffffffull) != static_cast<uint64_t>(b)) continue;
    pairs.push_back(static_cast<int32_t>(b));
    pairs.push_back(static_cast<int32_t>(m));
  }
}

// ---- CG4: hypotheses (host only) -------------------------------------------------------------------------------------------
// the generator: splitmix64's finaliser over the counter 3 h + slot + 1, the high 32 bits scaled onto 0 .. C - 1
inline int64_t draw(uint64_t seed, uint32_t h, uint32_t slot, int64_t C) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (3ull * h + slot + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return static_cast<int64_t>(((z >> 32) * static_cast<uint64_t>(C)) >> 32);
}

struct Hypothesis {
  int32_t code, triple[3];
  rg::Frame f;
};

inline double norm3(const double v[3]) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
inline void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// one triangle: its sides' lengths (12, 13, 23), its frame (e1, e2, e3 as rows) and its centroid; false = thinner than CG4 allows
inline bool triangle_of(const float *p1, const float *p2, const float *p3, double min_sin2, double len[3], double e[9], double cen[3]) {
  double a[3], b[3], c[3], n[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = static_cast<double>(p2[k]) - static_cast<double>(p1[k]);
    b[k] = static_cast<double>(p3[k]) - static_cast<double>(p1[k]);
    c[k] = static_cast<double>(p3[k]) - static_cast<double>(p2[k]);
    cen[k] = ((static_cast<double>(p1[k]) + static_cast<double>(p2[k])) + static_cast<double>(p3[k])) / 3.0;
  }
  len[0] = norm3(a), len[1] = norm3(b), len[2] = norm3(c);
  cross3(a, b, n);
  const double n2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  // the smallest angle lies between the two longest sides: |a x b| = (their product) * its sine
  const double s0 = len[0] * len[0], s1 = len[1] * len[1], s2 = len[2] * len[2];
  const double least = std::fmin(s0, std::fmin(s1, s2));
  const double bound = min_sin2 * (((s0 * s1) * s2) / least);
  if (!(n2 > 0.0) || !(n2 >= bound)) return false;
  const double nl = std::sqrt(n2);
  for (int k = 0; k < 3; ++k) e[k] = a[k] / len[0], e[6 + k] = n[k] / nl;
  cross3(e + 6, e, e + 3);
  return true;
}

// CG4 for hypothesis h over C >= 1 correspondences (cb, cm: 3 floats each), as a frame about `pivot`
inline void hypothesis(const Rule &r, int64_t C, const float *cb, const float *cm, const double pivot[3], uint32_t h, Hypothesis &out) {
  for (int s = 0; s < 3; ++s) out.triple[s] = static_cast<int32_t>(draw(r.seed, h, static_cast<uint32_t>(s), C));
  out.code = kAccepted;
  for (int a = 0; a < 9; ++a) out.f.R[a] = (a % 4 == 0) ? 1.0 : 0.0;
  for (int a = 0; a < 3; ++a) out.f.c[a] = pivot[a], out.f.t[a] = 0.0;
  const int32_t *t = out.triple;
  if (t[0] == t[1] || t[0] == t[2] || t[1] == t[2]) {
    out.code = kRepeat;
    return;
  }
  double lm[3], lb[3], em[9], eb[9], cenm[3], cenb[3];
  const bool okm = triangle_of(cm + 3 * t[0], cm + 3 * t[1], cm + 3 * t[2], r.min_sin2, lm, em, cenm);
  const bool okb = triangle_of(cb + 3 * t[0], cb + 3 * t[1], cb + 3 * t[2], r.min_sin2, lb, eb, cenb);
  for (int s = 0; s < 3; ++s)
    if (!(lm[s] >= r.min_side)) {
      out.code = kShortSide;
      return;
    }
  for (int s = 0; s < 3; ++s)
    if (!(std::fabs(lm[s] - lb[s]) <= r.side_tolerance)) {
      out.code = kSideMismatch;
      return;
    }
  if (!okm || !okb) {
    out.code = kThin;
    return;
  }
  // R = F_map F_base^T, the frames' vectors as columns
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out.f.R[3 * i + j] = (em[i] * eb[j] + em[3 + i] * eb[3 + j]) + em[6 + i] * eb[6 + j];
  double d[3];
  for (int a = 0; a < 3; ++a) d[a] = cenb[a] - pivot[a];
  for (int a = 0; a < 3; ++a) {
    const double rd = (out.f.R[3 * a] * d[0] + out.f.R[3 * a + 1] * d[1]) + out.f.R[3 * a + 2] * d[2];
    out.f.t[a] = (cenm[a] - pivot[a]) - rd;
  }
}

// ---- CG5: scoring ----------------------------------------------------------------------------------------------------------
// the offset d = map partner - moved base keypoint, each component fl32
PCP_RG_HD bool inlier_of(int64_t tau2, float dx, float dy, float dz) {
  if (!(fabsf(dx) <= 1.0f && fabsf(dy) <= 1.0f && fabsf(dz) <= 1.0f)) return false;  // (NaN too; keeps the quanta inside int32)
  const int64_t qx = gn::quantise(dx), qy = gn::quantise(dy), qz = gn::quantise(dz);
  return (qx * qx + qy * qy) + qz * qz <= tau2;
}

PCP_RG_HD bool inlier_pair(const rg::Frame &f, int64_t tau2, const float *b, const float *m) {
  float o[3];
  rg::apply(f, b[0], b[1], b[2], o);
  return inlier_of(tau2, m[0] - o[0], m[1] - o[1], m[2] - o[2]);
}

// ---- CG6: consensus (host only) --------------------------------------------------------------------------------------------
inline int64_t refit_quantum(float v, double c) { return static_cast<int64_t>(std::rint((static_cast<double>(v) - c) * kRefitScale)); }

// Horn's quaternion solution over the flagged correspondences, as a frame about pivot_b.  0, or -1: a coordinate beyond
// kMaxRefit quanta of its pivot.  Fewer than 3 flagged pairs give the identity rotation.
inline int refit(int64_t C, const float *cb, const float *cm, const uint8_t *flags, const double pivot_b[3], const double pivot_m[3],
                 rg::Frame &f) {
  typedef __int128 wide;
  wide n = 0, su[3] = {0, 0, 0}, sv[3] = {0, 0, 0}, suv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t k = 0; k < C; ++k) {
    if (!flags[k]) continue;
    int64_t u[3], v[3];
    for (int a = 0; a < 3; ++a) {
      u[a] = refit_quantum(cb[3 * k + a], pivot_b[a]);
      v[a] = refit_quantum(cm[3 * k + a], pivot_m[a]);
      if (u[a] < -kMaxRefit || u[a] > kMaxRefit || v[a] < -kMaxRefit || v[a] > kMaxRefit) return -1;
    }
    n += 1;
    for (int a = 0; a < 3; ++a) {
      su[a] += u[a], sv[a] += v[a];
      for (int b = 0; b < 3; ++b) suv[3 * a + b] += static_cast<wide>(u[a]) * v[b];
    }
  }
  for (int a = 0; a < 9; ++a) f.R[a] = (a % 4 == 0) ? 1.0 : 0.0;
  for (int a = 0; a < 3; ++a) f.c[a] = pivot_b[a], f.t[a] = 0.0;
  if (n < 3) return 0;
  const double dn = static_cast<double>(n);
  double S[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) S[3 * a + b] = (static_cast<double>(n * suv[3 * a + b] - su[a] * sv[b]) / dn) / 4294967296.0;
  double A[4][4], V[4][4];
  A[0][0] = (S[0] + S[4]) + S[8];
  A[0][1] = S[5] - S[7], A[0][2] = S[6] - S[2], A[0][3] = S[1] - S[3];
  A[1][1] = (S[0] - S[4]) - S[8];
  A[1][2] = S[1] + S[3], A[1][3] = S[6] + S[2];
  A[2][2] = (S[4] - S[0]) - S[8];
  A[2][3] = S[5] + S[7];
  A[3][3] = (S[8] - S[0]) - S[4];
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < a; ++b) A[a][b] = A[b][a];
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) V[a][b] = a == b ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kSweeps; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int i = 0; i < 4; ++i) {
          const double aip = A[i][p], aiq = A[i][q];
          A[i][p] = c * aip - sn * aiq;
          A[i][q] = sn * aip + c * aiq;
        }
        for (int i = 0; i < 4; ++i) {
          const double api = A[p][i], aqi = A[q][i];
          A[p][i] = c * api - sn * aqi;
          A[q][i] = sn * api + c * aqi;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int i = 0; i < 4; ++i) {
          const double vip = V[i][p], viq = V[i][q];
          V[i][p] = c * vip - sn * viq;
          V[i][q] = sn * vip + c * viq;
        }
      }
  int top = 0;
  for (int a = 1; a < 4; ++a)
    if (A[a][a] > A[top][top]) top = a;
  double q[4] = {V[0][top], V[1][top], V[2][top], V[3][top]};
  const double len = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  if (!(len > 0.0)) return 0;
  const double sign = q[0] < 0.0 ? -1.0 : 1.0;
  for (int a = 0; a < 4; ++a) q[a] = (q[a] / len) * sign;
  rg::rotation_of(q, f.R);
  double mu[3], mv[3];
  for (int a = 0; a < 3; ++a) {
    mu[a] = (static_cast<double>(su[a]) / dn) / kRefitScale;
    mv[a] = (static_cast<double>(sv[a]) / dn) / kRefitScale;
  }
  for (int a = 0; a < 3; ++a) {
    const double rd = (f.R[3 * a] * mu[0] + f.R[3 * a + 1] * mu[1]) + f.R[3 * a + 2] * mu[2];
    f.t[a] = ((pivot_m[a] - pivot_b[a]) + mv[a]) - rd;
  }
  return 0;
}

inline double trace_between(const double A[9], const double B[9]) {
  double s = 0.0;
  for (int a = 0; a < 9; ++a) s = s + A[a] * B[a];
  return s;
}

// CG4-CG6 around a scoring `score(frames, n_frames, counts, flags) -> int` (0, or the error to pass on; flags nullable: the
// inlier bytes of the ONE frame given): the host form and the device form differ in the scoring alone.  report: words kScored
// .. kTriple2 are written (the caller fills the five before).  found: the frame that was kept (status 0 only).  inliers: C bytes
// of the kept frame.  -1: the refit's range.
template <class Score>
inline int consensus(const Rule &r, int64_t C, const float *cb, const float *cm, const double pivot_b[3], const double pivot_m[3], Score score,
                     int64_t report[kReportWords], rg::Frame *found, std::vector<uint8_t> &inliers) {
  for (int a = kScored; a < kReportWords; ++a) report[a] = 0;
  report[kStatus] = kTooFewInliers;
  report[kWinnerH] = report[kTriple0] = report[kTriple1] = report[kTriple2] = -1;
  inliers.assign(static_cast<size_t>(C), 0);
  if (C < 3) return 0;
  std::vector<rg::Frame> frames;
  std::vector<int32_t> which;
  std::vector<Hypothesis> hyp(static_cast<size_t>(r.hypotheses));
  for (int32_t h = 0; h < r.hypotheses; ++h) {
    hypothesis(r, C, cb, cm, pivot_b, static_cast<uint32_t>(h), hyp[static_cast<size_t>(h)]);
    if (hyp[static_cast<size_t>(h)].code != kAccepted) continue;
    frames.push_back(hyp[static_cast<size_t>(h)].f);
    which.push_back(h);
  }
  report[kScored] = static_cast<int64_t>(frames.size());
  report[kRefused] = r.hypotheses - report[kScored];
  if (frames.empty()) return 0;
  std::vector<int64_t> counts(frames.size(), 0);
  int rc = score(frames.data(), static_cast<int64_t>(frames.size()), counts.data(), static_cast<uint8_t *>(nullptr));
  if (rc != 0) return rc;
  size_t win = 0;
  for (size_t k = 1; k < frames.size(); ++k)
    if (counts[k] > counts[win]) win = k;
  report[kWinner] = counts[win];
  for (size_t k = 0; k < frames.size(); ++k)
    if (trace_between(frames[k].R, frames[win].R) < kRunnerTrace && counts[k] > report[kRunnerUp]) report[kRunnerUp] = counts[k];
  report[kWinnerH] = which[win];
  for (int s = 0; s < 3; ++s) report[kTriple0 + s] = hyp[static_cast<size_t>(which[win])].triple[s];
  if (counts[win] < r.min_inliers) return 0;
  int64_t one = 0;
  if ((rc = score(&frames[win], 1, &one, inliers.data())) != 0) return rc;
  rg::Frame again;
  if (refit(C, cb, cm, inliers.data(), pivot_b, pivot_m, again) != 0) return -1;
  std::vector<uint8_t> flags(static_cast<size_t>(C), 0);
  if ((rc = score(&again, 1, &one, flags.data())) != 0) return rc;
  report[kRefit] = one;
  *found = frames[win];
  report[kKept] = counts[win];
  if (one >= counts[win]) {
    *found = again;
    report[kKept] = one;
    inliers.swap(flags);
  }
  report[kStatus] = kFound;
  return 0;
}

// CG7: the frame as the row-major 4 x 4 that pcp_compare_set_base_transform takes
inline void matrix_of_frame(const rg::Frame &f, double M[16]) {
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) M[4 * a + b] = f.R[3 * a + b];
    const double rc = (f.R[3 * a] * f.c[0] + f.R[3 * a + 1] * f.c[1]) + f.R[3 * a + 2] * f.c[2];
    M[4 * a + 3] = (f.c[a] - rc) + f.t[a];
  }
  M[12] = M[13] = M[14] = 0.0;
  M[15] = 1.0;
}

}  // namespace cg
}  // namespace pcp
