// pcp_voxel_reduce.hpp -- the arithmetic of the voxel-grid output ("Voxel-grid output", VG1-VG7), one copy for
// the kernels (pcp_voxel_reduce.hip), the CPU form (pcp_voxel_reduce_host) and the host self-test
// (host/voxel_reduce_selftest.cpp).  Exact integers throughout: a voxel's result is a function of the SET of its rows, so
// it cannot depend on the order of rows, chunks or atomics.  Build without floating-point contraction (no product here
// feeds a sum, but the rule of the library holds for this file too).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCP_VG_HD __host__ __device__ __forceinline__
#else
#define PCP_VG_HD inline
#endif

namespace pcp {
namespace vg {

constexpr int32_t kCellBias = 1 << 20;        // VG3: |cell| < 2^20 on every axis
constexpr uint32_t kMaxRowsPerVoxel = 1u << 24;  // VG6: a voxel with this many rows or more is refused at the finish
constexpr uint64_t kNoKey = ~uint64_t(0);     // never a key: keys are 63 bits

// VG1: finite, 1e-4 <= leaf <= 1 (both bounds as fp32)
PCP_VG_HD bool leaf_ok(float leaf) { return leaf >= 1e-4f && leaf <= 1.0f; }
PCP_VG_HD float inverse_leaf(float leaf) { return 1.0f / leaf; }

// VG3: the cell of one coordinate, floorf of the fp32 product; false for a non-finite coordinate or |cell| >= 2^20
PCP_VG_HD bool cell_of(float x, float inv, int32_t *c) {
  const float p = x * inv;
  const float f = floorf(p);
  if (!(fabsf(f) < 1048576.0f)) return false;  // (NaN and +-inf fail the comparison)
  *c = static_cast<int32_t>(f);
  return true;
}

// VG4: x fastest, z slowest (PCL's leaf-index order)
PCP_VG_HD uint64_t key_of(int32_t cx, int32_t cy, int32_t cz) {
  return (static_cast<uint64_t>(cz + kCellBias) << 42) | (static_cast<uint64_t>(cy + kCellBias) << 21) |
         static_cast<uint64_t>(cx + kCellBias);
}
PCP_VG_HD void cells_of_key(uint64_t key, int32_t *cx, int32_t *cy, int32_t *cz) {
  *cx = static_cast<int32_t>(key & 0x1fffffu) - kCellBias;
  *cy = static_cast<int32_t>((key >> 21) & 0x1fffffu) - kCellBias;
  *cz = static_cast<int32_t>((key >> 42) & 0x1fffffu) - kCellBias;
}

// round to nearest, ties to even, of a double below 2^63 in magnitude
PCP_VG_HD int64_t round_ll(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __double2ll_rn(v);
#else
  return static_cast<int64_t>(llrint(v));  // (the default rounding mode; nothing in the library changes it)
#endif
}

// VG5: the corner of a cell and a coordinate in units of 2^-32 m.  Both products are exact in fp64 (21 x 24 bits; a power
// of two), the rounding is round_ll's.
PCP_VG_HD int64_t corner_of(int32_t c, float leaf) {
  return round_ll(static_cast<double>(c) * static_cast<double>(leaf) * 4294967296.0);
}
PCP_VG_HD int64_t fixed_of(float x) { return round_ll(static_cast<double>(x) * 4294967296.0); }

PCP_VG_HD int64_t floor_div(int64_t a, int64_t b /* > 0 */) {
  const int64_t q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// VG7: the centroid coordinate of a voxel from the sum of its rows' offsets from the corner
PCP_VG_HD float centroid_of(int32_t c, float leaf, int64_t sum_q, uint32_t n) {
  const int64_t n64 = static_cast<int64_t>(n);
  const int64_t fix = corner_of(c, leaf) + floor_div(2 * sum_q + n64, 2 * n64);
  return static_cast<float>(static_cast<double>(fix) * (1.0 / 4294967296.0));
}

// one row of the result from a voxel's sums (n > 0)
struct Sums {
  int64_t q[3];
  uint32_t n, r, g, b, label;
};
PCP_VG_HD void finish_voxel(uint64_t key, float leaf, const Sums &s, float xyz[3], uint8_t rgb[3], uint8_t *label) {
  int32_t c[3];
  cells_of_key(key, &c[0], &c[1], &c[2]);
  for (int a = 0; a < 3; ++a) xyz[a] = centroid_of(c[a], leaf, s.q[a], s.n);
  rgb[0] = static_cast<uint8_t>(s.r / s.n);
  rgb[1] = static_cast<uint8_t>(s.g / s.n);
  rgb[2] = static_cast<uint8_t>(s.b / s.n);
  *label = static_cast<uint8_t>(s.label / s.n);
}

}  // namespace vg
}  // namespace pcp
