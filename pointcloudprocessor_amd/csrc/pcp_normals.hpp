// pcp_normals.hpp -- the integer part of the map normals ("Geometry maps", GN2-GN5), one copy for the kernel
// (pcp_normals.hip), the CPU form (pcp_normals_moments_host) and the host self-test (host/normals_selftest.cpp).  A
// neighbour's offset from the query is quantised to 2^-20 m and the moments are exact 64-bit integer sums, so they are a
// function of the SET of neighbours: no dependence on the order of the neighbours, the grid, the cell size or the input
// order.  Build without floating-point contraction: every fp32 / fp64 operation below is rounded on its own.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCP_GN_HD __host__ __device__ __forceinline__
#else
#define PCP_GN_HD inline
#endif

namespace pcp {
namespace gn {

constexpr float kQuantaPerMetre = 1048576.0f;        // GN3: 2^20, the quantum is ~0.95 um
constexpr int32_t kMaxQuantum = (1 << 20) + 1;        // GN4: |q| <= 2^20 + 1 for an accepted offset (r <= 1)
constexpr int64_t kMaxNeighbours = int64_t(1) << 22;  // GN4: a point with this many neighbours or more is PCP_ERR_RANGE
constexpr int32_t kMinNeighbours = 3;                 // GN7
constexpr int kMomentWords = 10;                      // n S1x S1y S1z S2xx xy xz yy yz zz

// GN2: finite, 0.005 <= r <= 1 (both bounds as fp32)
PCP_GN_HD bool radius_ok(float r) { return r >= 0.005f && r <= 1.0f; }

// GN2 (LS2's threshold): the largest float t with (double)t <= (double)r * (double)r
inline float threshold_of(float r) {
  const double r2 = static_cast<double>(r) * static_cast<double>(r);
  float t = static_cast<float>(r2);
  if (static_cast<double>(t) > r2) t = std::nextafter(t, 0.0f);
  return t;
}

// GN1: three finite coordinates
PCP_GN_HD bool finite3(float x, float y, float z) {
  return fabsf(x) <= 3.402823466e+38f && fabsf(y) <= 3.402823466e+38f && fabsf(z) <= 3.402823466e+38f;
}

// GN3: rint(d * 2^20), ties to even, as int32.  The product is exact (a power of two, |d| <= ~1).
PCP_GN_HD int32_t quantise(float d) {
  const float p = d * kQuantaPerMetre;
#if defined(__HIP_DEVICE_COMPILE__)
  return __float2int_rn(p);
#else
  return static_cast<int32_t>(lrintf(p));  // (the default rounding mode; nothing in the library changes it)
#endif
}

// GN4: the moments of one query about itself
struct Moments {
  int64_t n;
  int64_t s1[3];
  int64_t s2[6];  // xx xy xz yy yz zz
};

PCP_GN_HD void clear(Moments &m) {
  m.n = 0;
  for (int a = 0; a < 3; ++a) m.s1[a] = 0;
  for (int a = 0; a < 6; ++a) m.s2[a] = 0;
}

// GN2-GN4 for one candidate: the fp32 test on d = candidate - query, then the integer adds; true iff it was a neighbour
PCP_GN_HD bool visit(Moments &m, float dx, float dy, float dz, float t) {
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  if (!(d2 <= t)) return false;
  const int32_t qx = quantise(dx), qy = quantise(dy), qz = quantise(dz);
  m.n += 1;
  m.s1[0] += qx;
  m.s1[1] += qy;
  m.s1[2] += qz;
  m.s2[0] += static_cast<int64_t>(qx) * qx;
  m.s2[1] += static_cast<int64_t>(qx) * qy;
  m.s2[2] += static_cast<int64_t>(qx) * qz;
  m.s2[3] += static_cast<int64_t>(qy) * qy;
  m.s2[4] += static_cast<int64_t>(qy) * qz;
  m.s2[5] += static_cast<int64_t>(qz) * qz;
  return true;
}

// GN5: C_ab = (double)S2_ab - ((double)S1_a * (double)S1_b) / (double)n, three IEEE operations per entry (n > 0)
PCP_GN_HD void covariance(const Moments &m, double C[6]) {
  const double n = static_cast<double>(m.n);
  const double sx = static_cast<double>(m.s1[0]), sy = static_cast<double>(m.s1[1]), sz = static_cast<double>(m.s1[2]);
  C[0] = static_cast<double>(m.s2[0]) - (sx * sx) / n;
  C[1] = static_cast<double>(m.s2[1]) - (sx * sy) / n;
  C[2] = static_cast<double>(m.s2[2]) - (sx * sz) / n;
  C[3] = static_cast<double>(m.s2[3]) - (sy * sy) / n;
  C[4] = static_cast<double>(m.s2[4]) - (sy * sz) / n;
  C[5] = static_cast<double>(m.s2[5]) - (sz * sz) / n;
}

PCP_GN_HD void store(const Moments &m, int64_t out[kMomentWords]) {
  out[0] = m.n;
  for (int a = 0; a < 3; ++a) out[1 + a] = m.s1[a];
  for (int a = 0; a < 6; ++a) out[4 + a] = m.s2[a];
}

}  // namespace gn
}  // namespace pcp
