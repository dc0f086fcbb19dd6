// pcp_tile_box.hpp -- how far the camera coordinates of a tile's points lie from those of its centre: the inflation of
// tile_classify_box (pcp_tile_classify.hpp), in a form that also compiles for the host (host/tile_bounds_selftest.cpp checks it
// against brute force).
//
// A tile's bound is its sphere {c, r} and the half-extents h of its world-axis box about c (pcp_context.hip k_up_bounds): every
// member p has |p - c| <= r and |p_j - c_j| <= h_j.  With M the 3x3 part of the fp32 matrix w2c and s a bound of its spectral
// norm, row r of M (p - c) obeys both
//   |(M (p - c))_r| <= |M (p - c)| <= s |p - c| <= s r                                    (the sphere: tile_classify's bound)
//   |(M (p - c))_r| = |sum_j m_rj (p_j - c_j)| <= sum_j |m_rj| |p_j - c_j| <= sum_j |m_rj| h_j      (the box)
// so the smaller of the two holds, row by row.  A tile is a patch of a surface: its box is flat where the sphere is round, and
// the row that looks along the flat direction gains most.  Each bound is inflated by 1 + 1e-6 (the fp64 rounding of its own
// evaluation) and by 1e-6 mag, which covers the fp32 rounding of the per-point transform x m0 + (y m1 + (z m2 + m3)): three
// products and three sums, each within 2^-24 of a partial sum that mag dominates (|m_rj| <= s, |p_j| <= |c_j| + r).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PCP_TB_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define PCP_TB_HD inline
#endif

namespace pcp {

struct TileInflation {
  double sphere;  // rho of tile_classify: the same for the three rows
  double row[3];  // min(sphere, the box's bound of the row)
};

// m: w2c, 3 x 4 row-major fp32; s: DevFrame::norm_bound; (cx, cy, cz, r): the sphere; (hx, hy, hz): the half-extents.
// A non-finite h (a member with an infinite coordinate) makes a row's sum infinite or NaN: fmin then returns the sphere's
// bound, which is infinite as well, and the classifier gives no verdict.
PCP_TB_HD TileInflation tile_inflation(const float *m, double s, double cx, double cy, double cz, double r, double hx, double hy,
                                       double hz) {
  const double mag = s * (fabs(cx) + fabs(cy) + fabs(cz) + 3.0 * r) + fabs(static_cast<double>(m[3])) +
                     fabs(static_cast<double>(m[7])) + fabs(static_cast<double>(m[11])) + 1e-3;
  const double slack = 1e-6 * mag;
  TileInflation t;
  t.sphere = s * r * (1.0 + 1e-6) + slack;
  for (int k = 0; k < 3; ++k) {
    const double box = (fabs(static_cast<double>(m[4 * k])) * hx + fabs(static_cast<double>(m[4 * k + 1])) * hy) +
                       fabs(static_cast<double>(m[4 * k + 2])) * hz;
    t.row[k] = fmin(t.sphere, box * (1.0 + 1e-6) + slack);
  }
  return t;
}

}  // namespace pcp
