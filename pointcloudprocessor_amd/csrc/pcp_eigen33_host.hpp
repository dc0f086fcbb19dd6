// pcp_eigen33_host.hpp -- pcl::eigen33's closed form on the host, in plain fp64 with the library's own libm: the eigenvalues of
// a symmetric 3 x 3 matrix and the eigenvector of one of them, for the host-only plane fits (pcp_ortho_fit_frame_host,
// pcp_facet_plane_host).  The device form is pcp_eigen33.hpp.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace pcp {
namespace eig {

inline void roots2(double b, double c, double r[3]) {
  double d = b * b - 4.0 * c;
  if (d < 0.0) d = 0.0;
  const double sd = std::sqrt(d);
  r[0] = 0.0;
  r[1] = 0.5 * (b - sd);
  r[2] = 0.5 * (b + sd);
}
// m = xx xy xz yy yz zz scaled to a largest magnitude of 1: its roots ascending
inline void roots3(const double a[6], double r[3]) {
  const double a00 = a[0], a01 = a[1], a02 = a[2], a11 = a[3], a12 = a[4], a22 = a[5];
  const double c0 = a00 * a11 * a22 + 2.0 * a01 * a02 * a12 - a00 * a12 * a12 - a11 * a02 * a02 - a22 * a01 * a01;
  const double c1 = a00 * a11 - a01 * a01 + a00 * a22 - a02 * a02 + a11 * a22 - a12 * a12;
  const double c2 = a00 + a11 + a22;
  if (std::fabs(c0) < DBL_EPSILON) return roots2(c2, c1, r);
  const double inv3 = 1.0 / 3.0, sqrt3 = std::sqrt(3.0);
  const double c2_3 = c2 * inv3;
  double a_3 = (c1 - c2 * c2_3) * inv3;
  if (a_3 > 0.0) a_3 = 0.0;
  const double half_b = 0.5 * (c0 + c2_3 * (2.0 * c2_3 * c2_3 - c1));
  double q = half_b * half_b + a_3 * a_3 * a_3;
  if (q > 0.0) q = 0.0;
  const double rho = std::sqrt(-a_3), theta = std::atan2(std::sqrt(-q), half_b) * inv3;
  const double ct = std::cos(theta), st = std::sin(theta);
  r[0] = c2_3 + 2.0 * rho * ct;
  r[1] = c2_3 - rho * (ct + sqrt3 * st);
  r[2] = c2_3 - rho * (ct - sqrt3 * st);
  std::sort(r, r + 3);
  if (r[0] <= 0.0) roots2(c2, c1, r);
}
// the unit eigenvector of root r: the longest cross product of two rows of (A - r I)
inline void eigenvector(const double a[6], double r, double v[3]) {
  const double a01 = a[1], a02 = a[2], a12 = a[4];
  const double s00 = a[0] - r, s11 = a[3] - r, s22 = a[5] - r;
  const double k[3][3] = {{a01 * a12 - a02 * s11, a02 * a01 - s00 * a12, s00 * s11 - a01 * a01},
                          {a01 * s22 - a02 * a12, a02 * a02 - s00 * s22, s00 * a12 - a01 * a02},
                          {s11 * s22 - a12 * a12, a12 * a02 - a01 * s22, a01 * a12 - s11 * a02}};
  int best = 0;
  double len[3];
  for (int i = 0; i < 3; ++i) {
    len[i] = (k[i][0] * k[i][0] + k[i][1] * k[i][1]) + k[i][2] * k[i][2];
    if (len[i] > len[best]) best = i;
  }
  const double inv = 1.0 / std::sqrt(len[best]);
  for (int c = 0; c < 3; ++c) v[c] = k[best][c] * inv;
}
inline int largest_component(const double v[3]) {
  int b = 0;
  for (int c = 1; c < 3; ++c)
    if (std::fabs(v[c]) > std::fabs(v[b])) b = c;
  return b;
}

}  // namespace eig
}  // namespace pcp
