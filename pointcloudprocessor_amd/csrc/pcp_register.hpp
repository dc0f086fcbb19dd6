// pcp_register.hpp -- the rule of the map registration ("Map registration", RG1-RG9), one copy for the kernels
// (pcp_register.hip), the CPU form (pcp_compare_register_host) and the host self-test (host/register_selftest.cpp).  The
// base survey is brought onto the map by point-to-plane ICP: per sampled base row the nearest map point (one 64-bit key
// minimised over the walk), thirty integer terms of the pair's normal equation, summed exactly as pairs of 64-bit halves, and
// a fixed sequence of fp64 operations (cyclic Jacobi on the 6 x 6, host only) that turns the sums into an update of the
// transform.  Build without floating-point contraction: every fp32 / fp64 operation below is rounded on its own.
//
// Ranges (RG4 / RG5).  match_radius <= 0.5 as in MC3, so an offset that passes the sphere test has every |q_a| <= 2^19 + 1
// and, with a valid normal (|N_a| <= 2^11, N2 <= 3 * 2^22), |h| = |q.N| < 1.74 * 2^30 < 2^31 and h^2 < 2^62 (pcp_compare.hpp's
// derivation).  The lever arm is |u_a| <= 2^18 quanta of 2^-8 m, so |(u x N)_a| <= 2 * 2^18 * 2^11 = 2^30 and every |g_a| <=
// 2^30: |g_a g_b| <= 2^60, |g_a h| < 2^61.  tau2 <= (0.5 * 2^20)^2 = 2^38 and tau2 * N2 <= 3 * 2^60 < 2^62.  Every term is
// below 2^62 in magnitude: its low 32 bits (unsigned) are below 2^32 and its arithmetic high part below 2^30 in magnitude.
// With fewer than 2^31 pairs the sum of the low parts is below 2^63 and that of the high parts below 2^61: no carries.
// terms_hold() re-derives the per-pair bounds in 128-bit arithmetic and the host form asserts it per pair.
#pragma once

#include <cmath>
#include <cstdint>

#include "pcp_compare.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCP_RG_HD __host__ __device__ __forceinline__
#define PCP_RG_UNROLL _Pragma("unroll")
#else
#define PCP_RG_HD inline
#define PCP_RG_UNROLL
#endif

namespace pcp {
namespace rg {

constexpr int kTerms = 30;                  // RG5: 21 g_a g_b (a <= b, row by row), 6 g_a h, h h, N2, 1
constexpr int kSumWords = 2 * kTerms;       // word 2 k: the low 32 bits summed, word 2 k + 1: the high parts summed
constexpr double kLeverScale = 256.0;       // RG4: the lever arm's quantum is 2^-8 m
constexpr int64_t kMaxLever = int64_t(1) << 18;
constexpr int kSweeps = 12;                 // RG6: cyclic Jacobi sweeps over the 15 pairs (p < q, row by row)
constexpr int kLogWords = 5;                // RG8: pairs, rms, dof, |omega| ell, |dt| per iteration
constexpr double kDefaultCondTol = 6.2e-3;  // RG6 ("Map registration", the two spectra)

enum Status : int32_t { kConverged = 0, kIterationLimit = 1, kTooFewPairs = 2 };

// what a call fixes for every pair
struct Rule {
  float match_radius, t;  // RG3's sphere
  int64_t tau2;           // RG4's trim, in squared offset quanta
  int32_t stride, max_iterations;
  int64_t min_pairs;
  double tolerance, cond_tol;
};

// RG3 / RG4 / RG7: the parameters' bounds; nullptr, or what is wrong.  NaN fails every test.
inline const char *prepare(float match_radius, float max_plane_distance, int32_t sample_stride, int32_t max_iterations,
                           int64_t min_pairs, double tolerance, double cond_tol, Rule *out) {
  if (!(match_radius >= mc::kMinExtent) || !(match_radius <= mc::kMaxSearch)) return "match_radius outside 0.005..0.5 (or not finite)";
  if (!(max_plane_distance > 0.0f) || !(max_plane_distance <= match_radius)) return "max_plane_distance outside (0, match_radius]";
  if (sample_stride < 1) return "sample_stride below 1";
  if (max_iterations < 1 || max_iterations > 1000) return "max_iterations outside 1..1000";
  if (min_pairs < 1) return "min_pairs below 1";
  if (!(tolerance >= 0.0) || !(tolerance <= 1.0)) return "tolerance outside 0..1";
  if (!(cond_tol > 0.0) || !(cond_tol < 1.0)) return "cond_tol outside (0, 1)";
  Rule r{};
  r.match_radius = match_radius;
  r.t = gn::threshold_of(match_radius);
  const double qd = static_cast<double>(max_plane_distance) * 1048576.0;  // (exact: a power of two)
  r.tau2 = static_cast<int64_t>(std::floor(qd * qd));                      // (exact: 48 bits at most)
  r.stride = sample_stride;
  r.max_iterations = max_iterations;
  r.min_pairs = min_pairs;
  r.tolerance = tolerance;
  r.cond_tol = cond_tol;
  *out = r;
  return nullptr;
}

// ---- RG1: the transform ----------------------------------------------------------------------------------------------------
// x' = R (x - c) + c + t, R from the unit quaternion q = (w, x, y, z)
struct Transform {
  double q[4], t[3];
};

PCP_RG_HD void set_identity(Transform &T) {
  T.q[0] = 1.0;
  T.q[1] = T.q[2] = T.q[3] = 0.0;
  T.t[0] = T.t[1] = T.t[2] = 0.0;
}

PCP_RG_HD bool is_identity(const Transform &T) {
  return T.q[0] == 1.0 && T.q[1] == 0.0 && T.q[2] == 0.0 && T.q[3] == 0.0 && T.t[0] == 0.0 && T.t[1] == 0.0 && T.t[2] == 0.0;
}

PCP_RG_HD void rotation_of(const double q[4], double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z);
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = 1.0 - 2.0 * (x * x + z * z);
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// what the transform kernel gets: the rotation, the pivot, the translation
struct Frame {
  double R[9], c[3], t[3];
};

// RG1's fixed sequence for one original row (the identity never comes here: its rows are the original bytes)
PCP_RG_HD void apply(const Frame &f, float x, float y, float z, float out[3]) {
  const double dx = static_cast<double>(x) - f.c[0], dy = static_cast<double>(y) - f.c[1], dz = static_cast<double>(z) - f.c[2];
  const double r0 = (f.R[0] * dx + f.R[1] * dy) + f.R[2] * dz;
  const double r1 = (f.R[3] * dx + f.R[4] * dy) + f.R[5] * dz;
  const double r2 = (f.R[6] * dx + f.R[7] * dy) + f.R[8] * dz;
  out[0] = static_cast<float>((r0 + f.c[0]) + f.t[0]);
  out[1] = static_cast<float>((r1 + f.c[1]) + f.t[1]);
  out[2] = static_cast<float>((r2 + f.c[2]) + f.t[2]);
}

// RG1: the pivot and the scale of a box (ell = half the diagonal; a box without extent scales by 1)
inline void pivot_of(const float mn[3], const float mx[3], double c[3], double *ell) {
  double e[3];
  for (int a = 0; a < 3; ++a) {
    c[a] = (static_cast<double>(mn[a]) + static_cast<double>(mx[a])) * 0.5;
    e[a] = static_cast<double>(mx[a]) - static_cast<double>(mn[a]);
  }
  const double half = std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) * 0.5;
  *ell = half > 0.0 ? half : 1.0;
}

// RG8: the row-major 4 x 4 of a transform about pivot c
inline void matrix_of(const Transform &T, const double c[3], double M[16]) {
  double R[9];
  rotation_of(T.q, R);
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) M[4 * a + b] = R[3 * a + b];
    const double rc = (R[3 * a] * c[0] + R[3 * a + 1] * c[1]) + R[3 * a + 2] * c[2];
    M[4 * a + 3] = (c[a] - rc) + T.t[a];
  }
  M[12] = M[13] = M[14] = 0.0;
  M[15] = 1.0;
}

// a caller's 4 x 4 as a transform about pivot c: false when it is no rigid motion (last row, orthonormal to 1e-9, det > 0)
inline bool from_matrix(const double M[16], const double c[3], Transform *out) {
  for (int a = 0; a < 16; ++a)
    if (!(std::fabs(M[a]) <= 1.0e300)) return false;
  if (M[12] != 0.0 || M[13] != 0.0 || M[14] != 0.0 || M[15] != 1.0) return false;
  double R[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[3 * a + b] = M[4 * a + b];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double dot = (R[3 * a] * R[3 * b] + R[3 * a + 1] * R[3 * b + 1]) + R[3 * a + 2] * R[3 * b + 2];
      if (!(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1.0e-9)) return false;
    }
  const double det = (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (!(det > 0.0)) return false;
  // Shepperd's branches: the largest of w, x, y, z is computed from the diagonal, the others from the off-diagonal sums
  double q[4];
  const double tr = (R[0] + R[4]) + R[8];
  if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
    const double s = std::sqrt(1.0 + tr) * 2.0;
    q[0] = 0.25 * s, q[1] = (R[7] - R[5]) / s, q[2] = (R[2] - R[6]) / s, q[3] = (R[3] - R[1]) / s;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    const double s = std::sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0;
    q[0] = (R[7] - R[5]) / s, q[1] = 0.25 * s, q[2] = (R[1] + R[3]) / s, q[3] = (R[2] + R[6]) / s;
  } else if (R[4] >= R[8]) {
    const double s = std::sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0;
    q[0] = (R[2] - R[6]) / s, q[1] = (R[1] + R[3]) / s, q[2] = 0.25 * s, q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = std::sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0;
    q[0] = (R[3] - R[1]) / s, q[1] = (R[2] + R[6]) / s, q[2] = (R[5] + R[7]) / s, q[3] = 0.25 * s;
  }
  const double len = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  if (!(len > 0.0)) return false;
  for (int a = 0; a < 4; ++a) out->q[a] = q[a] / len;
  for (int a = 0; a < 3; ++a) {
    const double rc = (R[3 * a] * c[0] + R[3 * a + 1] * c[1]) + R[3 * a + 2] * c[2];
    out->t[a] = (M[4 * a + 3] - c[a]) + rc;
  }
  return true;
}

// ---- RG3 / RG4: one pair ---------------------------------------------------------------------------------------------------
// RG3's key of one candidate at offset d = candidate - query: the bits of fl32(d2) above the candidate's index (d2 >= +0 and
// no NaN between finite neighbours, so the bits order as the values do)
PCP_RG_HD uint64_t key_of(float dx, float dy, float dz, uint32_t index) {
  const float d2 = (dx * dx + dy * dy) + dz * dz;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t bits = __float_as_uint(d2);
#else
  uint32_t bits;
  __builtin_memcpy(&bits, &d2, 4);
#endif
  return (static_cast<uint64_t>(bits) << 32) | index;
}

PCP_RG_HD float d2_of_key(uint64_t key) {
  const uint32_t bits = static_cast<uint32_t>(key >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(bits);
#else
  float d2;
  __builtin_memcpy(&d2, &bits, 4);
  return d2;
#endif
}

// MC1's test of a normal and MC2's quanta, unoriented; false = the partner makes no pair
PCP_RG_HD bool normal_of(float nx, float ny, float nz, int32_t N[3]) {
  if (!gn::finite3(nx, ny, nz)) return false;
  if (!(fabsf(nx) <= 1.0f && fabsf(ny) <= 1.0f && fabsf(nz) <= 1.0f)) return false;
  N[0] = mc::quantise_normal(nx);
  N[1] = mc::quantise_normal(ny);
  N[2] = mc::quantise_normal(nz);
  return N[0] != 0 || N[1] != 0 || N[2] != 0;
}

// RG4's lever arm of one axis: rint((b' - c) * 2^8), ties to even (the caller checks the box against kMaxLever)
PCP_RG_HD int64_t lever_of(float b, double c) { return static_cast<int64_t>(rint((static_cast<double>(b) - c) * kLeverScale)); }

struct Pair {
  int64_t g[6], h, N2;
};

// RG4 for the offset d = partner - b' (already inside RG3's sphere), the partner's quanta N and the lever arm u: false = trimmed
PCP_RG_HD bool pair_of(int64_t tau2, float dx, float dy, float dz, const int32_t N[3], const int64_t u[3], Pair &p) {
  const int64_t qx = gn::quantise(dx), qy = gn::quantise(dy), qz = gn::quantise(dz);
  const int64_t n0 = N[0], n1 = N[1], n2 = N[2];
  p.h = (qx * n0 + qy * n1) + qz * n2;
  p.N2 = (n0 * n0 + n1 * n1) + n2 * n2;
  p.g[0] = u[1] * n2 - u[2] * n1;
  p.g[1] = u[2] * n0 - u[0] * n2;
  p.g[2] = u[0] * n1 - u[1] * n0;
  p.g[3] = n0, p.g[4] = n1, p.g[5] = n2;
  return p.h * p.h <= tau2 * p.N2;
}

// RG5's thirty terms of one pair, in the order of the sums
PCP_RG_HD void terms_of(const Pair &p, int64_t term[kTerms]) {
  int k = 0;
PCP_RG_UNROLL
  for (int a = 0; a < 6; ++a)
PCP_RG_UNROLL
    for (int b = a; b < 6; ++b) term[k++] = p.g[a] * p.g[b];
PCP_RG_UNROLL
  for (int a = 0; a < 6; ++a) term[k++] = p.g[a] * p.h;
  term[k++] = p.h * p.h;
  term[k++] = p.N2;
  term[k++] = 1;
}

PCP_RG_HD int64_t low_of(int64_t term) { return static_cast<int64_t>(static_cast<uint64_t>(term) & 0xffffffffull); }
PCP_RG_HD int64_t high_of(int64_t term) { return term >> 32; }

// The ranges of the header comment for one pair, re-derived in 128-bit arithmetic.  (Host only.)
inline bool terms_hold(int64_t tau2, float dx, float dy, float dz, const int32_t N[3], const int64_t u[3]) {
  typedef __int128 wide;
  const wide lim62 = static_cast<wide>(1) << 62, lim30 = static_cast<wide>(1) << 30;
  const wide q[3] = {gn::quantise(dx), gn::quantise(dy), gn::quantise(dz)};
  const wide n[3] = {N[0], N[1], N[2]};
  const wide h = (q[0] * n[0] + q[1] * n[1]) + q[2] * n[2], N2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  const wide g[6] = {u[1] * n[2] - u[2] * n[1], u[2] * n[0] - u[0] * n[2], u[0] * n[1] - u[1] * n[0], n[0], n[1], n[2]};
  bool ok = h * h < lim62 && static_cast<wide>(tau2) * N2 < lim62;
  for (int a = 0; a < 6; ++a) {
    ok = ok && g[a] <= lim30 && g[a] >= -lim30 && g[a] * h < lim62 && g[a] * h > -lim62;
    for (int b = a; b < 6; ++b) ok = ok && g[a] * g[b] < lim62 && g[a] * g[b] > -lim62;
  }
  return ok;
}

// ---- RG6: the solve (host only) --------------------------------------------------------------------------------------------
inline double sum_of(const int64_t *sums, int k) { return static_cast<double>(sums[2 * k]) + 4294967296.0 * static_cast<double>(sums[2 * k + 1]); }

// RG8: rms = sqrt(sum h^2 / sum N2) / 2^20 in metres; 0 without pairs
inline double rms_of(const int64_t *sums) {
  const double hh = sum_of(sums, 27), nn = sum_of(sums, 28);
  return nn > 0.0 ? std::sqrt(hh / nn) / 1048576.0 : 0.0;
}

// The update (omega[3], dt[3]) from the sums: the normal equations with the rotation columns scaled by ell, cyclic Jacobi with
// kSweeps sweeps in a fixed pair order, the solution inside the span of the eigenvectors with lambda_k >= cond_tol *
// lambda_max (and lambda_k > 0).  eig: the six eigenvalues in the order of the diagonal.  Returns dof.
inline int32_t solve(const int64_t *sums, double ell, double cond_tol, double update[6], double eig[6]) {
  const double sr = 1.0 / (524288.0 * ell), st = 1.0 / 2048.0;
  double s[6] = {sr, sr, sr, st, st, st}, A[6][6], V[6][6], rhs[6];
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      A[a][b] = (sum_of(sums, k) * s[a]) * s[b];
      A[b][a] = A[a][b];
      ++k;
    }
  for (int a = 0; a < 6; ++a) rhs[a] = (sum_of(sums, 21 + a) * s[a]) * (1.0 / 2147483648.0);
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) V[a][b] = a == b ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kSweeps; ++sweep)
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int i = 0; i < 6; ++i) {
          const double aip = A[i][p], aiq = A[i][q];
          A[i][p] = c * aip - sn * aiq;
          A[i][q] = sn * aip + c * aiq;
        }
        for (int i = 0; i < 6; ++i) {
          const double api = A[p][i], aqi = A[q][i];
          A[p][i] = c * api - sn * aqi;
          A[q][i] = sn * api + c * aqi;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int i = 0; i < 6; ++i) {
          const double vip = V[i][p], viq = V[i][q];
          V[i][p] = c * vip - sn * viq;
          V[i][q] = sn * vip + c * viq;
        }
      }
  double top = 0.0;
  for (int a = 0; a < 6; ++a) {
    eig[a] = A[a][a];
    if (eig[a] > top) top = eig[a];
  }
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int32_t dof = 0;
  const double floor_ = cond_tol * top;
  for (int e = 0; e < 6; ++e) {
    if (!(eig[e] > 0.0) || !(eig[e] >= floor_)) continue;
    ++dof;
    double dot = 0.0;
    for (int b = 0; b < 6; ++b) dot = dot + V[b][e] * rhs[b];
    const double coef = dot / eig[e];
    for (int a = 0; a < 6; ++a) x[a] = x[a] + V[a][e] * coef;
  }
  for (int a = 0; a < 3; ++a) update[a] = x[a] / ell;
  for (int a = 3; a < 6; ++a) update[a] = x[a];
  return dof;
}

// RG6: the update composed onto T (rotation about the pivot first, then the shift), the quaternion renormalised
inline void compose(Transform &T, const double update[6]) {
  const double hx = update[0] * 0.5, hy = update[1] * 0.5, hz = update[2] * 0.5;
  const double len = std::sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
  const double d[4] = {1.0 / len, hx / len, hy / len, hz / len};
  const double *q = T.q;
  double r[4];
  r[0] = ((d[0] * q[0] - d[1] * q[1]) - d[2] * q[2]) - d[3] * q[3];
  r[1] = ((d[0] * q[1] + d[1] * q[0]) + d[2] * q[3]) - d[3] * q[2];
  r[2] = ((d[0] * q[2] - d[1] * q[3]) + d[2] * q[0]) + d[3] * q[1];
  r[3] = ((d[0] * q[3] + d[1] * q[2]) - d[2] * q[1]) + d[3] * q[0];
  const double rl = std::sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);
  for (int a = 0; a < 4; ++a) T.q[a] = r[a] / rl;
  double Rd[9], t[3];
  rotation_of(d, Rd);
  for (int a = 0; a < 3; ++a) t[a] = ((Rd[3 * a] * T.t[0] + Rd[3 * a + 1] * T.t[1]) + Rd[3 * a + 2] * T.t[2]) + update[3 + a];
  for (int a = 0; a < 3; ++a) T.t[a] = t[a];
}

// RG7: the two sizes of an update, in metres
inline void sizes_of(const double update[6], double ell, double *rot, double *shift) {
  *rot = std::sqrt((update[0] * update[0] + update[1] * update[1]) + update[2] * update[2]) * ell;
  *shift = std::sqrt((update[3] * update[3] + update[4] * update[4]) + update[5] * update[5]);
}

// RG4: the lever arms of a box's faces stay inside kMaxLever
inline bool levers_hold(const float mn[3], const float mx[3], const double c[3]) {
  for (int a = 0; a < 3; ++a) {
    const int64_t lo = lever_of(mn[a], c[a]), hi = lever_of(mx[a], c[a]);
    if (lo < -kMaxLever || lo > kMaxLever || hi < -kMaxLever || hi > kMaxLever) return false;
  }
  return true;
}

// RG7's loop around an evaluation `eval(T, sums60) -> int` (PCP_OK = 0, or the error to pass on): the host form and the
// device form differ in the evaluation alone.  log: max_iterations rows of kLogWords; status2: the status, the rows written.
template <class Eval>
inline int iterate(const Rule &r, double ell, Transform &T, Eval eval, int64_t sums[kSumWords], double *log, int32_t status2[2]) {
  status2[0] = kIterationLimit;
  status2[1] = 0;
  for (int32_t it = 0; it < r.max_iterations; ++it) {
    const int rc = eval(T, sums);
    if (rc != 0) return rc;
    double *row = log + static_cast<size_t>(it) * kLogWords;
    const int64_t pairs = sums[2 * 29];
    row[0] = static_cast<double>(pairs);
    row[1] = rms_of(sums);
    row[2] = row[3] = row[4] = 0.0;
    status2[1] = it + 1;
    if (pairs < r.min_pairs) {
      status2[0] = kTooFewPairs;
      return 0;
    }
    double update[6], eig[6];
    row[2] = static_cast<double>(solve(sums, ell, r.cond_tol, update, eig));
    sizes_of(update, ell, &row[3], &row[4]);
    compose(T, update);
    if (row[3] < r.tolerance && row[4] < r.tolerance) {
      status2[0] = kConverged;
      return 0;
    }
  }
  return 0;
}

}  // namespace rg
}  // namespace pcp
