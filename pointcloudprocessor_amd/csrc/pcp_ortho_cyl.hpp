// pcp_ortho_cyl.hpp -- the per-element arithmetic of the unrolled maps of cylindrical facets ("Cylindrical
// facets", CY1-CY9), one copy for the kernels (pcp_ortho.hip), the CPU form (pcp_ortho_cyl_host), the fit
// (pcp_cyl_fit_host) and host/ortho_cyl_selftest.cpp.  Built with -ffp-contract=off: every product, sum, quotient and root
// below is rounded on its own, in the width its operands have.  Everything after the pixel is pcp_ortho.hpp's.
// The way back, from a fine pixel of an orthophoto to its surface point ("Orthophotos of unrolled maps", CT1-CT2), is here
// too: one copy for k_ortho_texture<true>, pcp_ortho_texture_points_cyl_host and host/ortho_cyl_texture_selftest.cpp.
#pragma once

#include "pcp_ortho.hpp"

namespace pcp {
namespace cy {

constexpr double kPi4 = 0x1.921fb54442d18p-1;  // the doubles nearest pi/4, pi/2, pi, 2 pi
constexpr double kPi2 = 0x1.921fb54442d18p+0;
constexpr double kPi = 0x1.921fb54442d18p+1;
constexpr double kTwoPi = 0x1.921fb54442d18p+2;
constexpr double kTan8 = 0x1.a827999fcef32p-2;  // tan(pi/8)
constexpr float kMinRadius = 0.05f, kMaxRadius = 1000.0f;  // CY1

// CY1: the frame as the kernels take it (the caller's values, inv = f32(1.0f / gsd), R and side promoted once)
struct Frame {
  float c[3], a[3], e[3], b[3];
  float inv, wf, hf, d_min, d_max;
  int32_t w, h;
  double R, side;
};

// CY3: the angle of (S, T) in [0, 2 pi] by one fixed sequence of fp64 operations: the quotient of the smaller by the larger
// magnitude, reduced about tan(pi/8), the arctangent's series to z^12 by Horner, and the unfolding over the octants.
// (0, 0) gives a NaN (0 / 0): CY2 never asks for it.
PCP_OM_HD double angle(double S, double T) {
  const double x = fabs(S), y = fabs(T);
  const bool steep = y > x;
  const double m = steep ? x : y, M = steep ? y : x;
  const double q = m / M;
  double r = q, base = 0.0;
  if (q > kTan8) {
    r = (q - 1.0) / (q + 1.0);
    base = kPi4;
  }
  const double z = r * r;
  double P = 1.0 / 25.0;
  P = P * z + -1.0 / 23.0;
  P = P * z + 1.0 / 21.0;
  P = P * z + -1.0 / 19.0;
  P = P * z + 1.0 / 17.0;
  P = P * z + -1.0 / 15.0;
  P = P * z + 1.0 / 13.0;
  P = P * z + -1.0 / 11.0;
  P = P * z + 1.0 / 9.0;
  P = P * z + -1.0 / 7.0;
  P = P * z + 1.0 / 5.0;
  P = P * z + -1.0 / 3.0;
  P = P * z + 1.0;
  double phi = base + r * P;
  if (steep) phi = kPi2 - phi;
  if (S < 0.0) phi = kPi - phi;
  if (T < 0.0) phi = kTwoPi - phi;
  return phi;
}

// CY2: pixel and depth bits of a point; false: not a contributor (the has bit is the caller's to check).  x comes from the
// arc R theta in fp64, y from the height along the axis in fp32, the depth from rho - R; the comparisons against the raster are
// made in float before any conversion; a depth of -0 leaves as +0; a point on the axis (rho = 0) never contributes.
// (coords: the three values before the tests, which the fit sizes its raster and window by; false: non-finite or on the axis)
PCP_OM_HD bool coords(const Frame &f, float px, float py, float pz, float *x, float *y, float *depth) {
  if (!(om::finite_bits(px) && om::finite_bits(py) && om::finite_bits(pz))) return false;
  const float d[3] = {px - f.c[0], py - f.c[1], pz - f.c[2]};
  const float s = om::dot3(d, f.e), t = om::dot3(d, f.b), h = om::dot3(d, f.a);
  const double S = static_cast<double>(s), T = static_cast<double>(t);
  const double rho = sqrt(S * S + T * T);
  if (!(rho > 0.0)) return false;
  const double arc = f.R * angle(S, T);
  *x = static_cast<float>(arc * static_cast<double>(f.inv));
  *y = h * f.inv;
  *depth = static_cast<float>(f.side * (rho - f.R));
  return true;
}
PCP_OM_HD bool project(const Frame &f, float px, float py, float pz, int32_t *pixel, uint32_t *depth_bits) {
  float x, y, depth;
  if (!coords(f, px, py, pz, &x, &y, &depth)) return false;
  if (!(x >= 0.0f && x < f.wf && y >= 0.0f && y < f.hf)) return false;
  if (!(depth >= f.d_min && depth <= f.d_max)) return false;
  const int32_t col = static_cast<int32_t>(floorf(x)), row = static_cast<int32_t>(floorf(y));
  *pixel = row * f.w + col;
  const uint32_t db = om::float_bits(depth);
  *depth_bits = (db & 0x7fffffffu) ? db : 0u;
  return true;
}

// CT1 ("Orthophotos of unrolled maps"): sine and cosine of 0 <= theta < 64 by one fixed sequence of fp64 operations:
// the nearest multiple k of pi/2, r = theta - k pi/2, both series to r^17 / r^16 by Horner, and the unfolding over k & 3.
// Each coefficient is one correctly rounded quotient (every factorial up to 17! is an exact double).
constexpr double kTwoOverPi = 0x1.45f306dc9c883p-1;  // the double nearest 2 / pi
PCP_OM_HD void sincos(double theta, double *s, double *c) {
  const int k = static_cast<int>(theta * kTwoOverPi + 0.5);
  const double r = theta - static_cast<double>(k) * kPi2;
  const double z = r * r;
  double S = 1.0 / 355687428096000.0;
  S = S * z + -1.0 / 1307674368000.0;
  S = S * z + 1.0 / 6227020800.0;
  S = S * z + -1.0 / 39916800.0;
  S = S * z + 1.0 / 362880.0;
  S = S * z + -1.0 / 5040.0;
  S = S * z + 1.0 / 120.0;
  S = S * z + -1.0 / 6.0;
  S = S * z + 1.0;
  S = r * S;
  double C = 1.0 / 20922789888000.0;
  C = C * z + -1.0 / 87178291200.0;
  C = C * z + 1.0 / 479001600.0;
  C = C * z + -1.0 / 3628800.0;
  C = C * z + 1.0 / 40320.0;
  C = C * z + -1.0 / 720.0;
  C = C * z + 1.0 / 24.0;
  C = C * z + -1.0 / 2.0;
  C = C * z + 1.0;
  switch (k & 3) {
    case 0: *s = S; *c = C; break;
    case 1: *s = C; *c = -S; break;
    case 2: *s = -S; *c = -C; break;
    default: *s = -C; *c = S; break;
  }
}

// CT2, the inverse of CY2: the position of the surface point of fine pixel (Xg, Yg) at scale k and depth d, fp64 from the
// frame's fp32 values and rounded to float once per coordinate.  xf / inv undoes CY2's x = arc inv.  false: rho <= 0, no surface.
PCP_OM_HD bool surface_point(const Frame &f, int32_t k, int32_t Xg, int32_t Yg, float d, float p[3]) {
  const double kd = static_cast<double>(k), inv = static_cast<double>(f.inv);
  const double xf = (static_cast<double>(Xg) + 0.5) / kd, yf = (static_cast<double>(Yg) + 0.5) / kd;
  const double arc = xf / inv, hh = yf / inv;
  const double theta = arc / f.R;
  const double rho = f.R + f.side * static_cast<double>(d);
  if (!(rho > 0.0)) return false;
  double s, c;
  sincos(theta, &s, &c);
  const double rc = rho * c, rs = rho * s;
  for (int a = 0; a < 3; ++a)
    p[a] = static_cast<float>(static_cast<double>(f.c[a]) +
                              ((rc * static_cast<double>(f.e[a]) + rs * static_cast<double>(f.b[a])) + hh * static_cast<double>(f.a[a])));
  return true;
}

// the frame as the kernels take it, from a pcp_cyl_frame (CY1)
template <class CFrame>
inline Frame make_frame(const CFrame &c) {
  Frame f;
  for (int k = 0; k < 3; ++k) {
    f.c[k] = c.c[k];
    f.a[k] = c.a[k];
    f.e[k] = c.e[k];
    f.b[k] = c.b[k];
  }
  f.inv = om::inverse_gsd(c.gsd);
  f.w = c.width;
  f.h = c.height;
  f.wf = static_cast<float>(c.width);
  f.hf = static_cast<float>(c.height);
  f.d_min = c.d_min;
  f.d_max = c.d_max;
  f.R = static_cast<double>(c.radius);
  f.side = static_cast<double>(c.side);
  return f;
}

// CY1, host only, with om::frame_check's codes.  0: fine; 1: a non-finite value, a gsd outside [1e-4, 1], a radius outside
// [0.05, 1000], a side that is not +-1, an empty raster or window, axes (e, b, a) that are not orthonormal with e x b = side a
// within 1e-3, a raster wider than the circumference plus a pixel (*why says which); 2: a raster past OM1's limits, *fit_gsd =
// the gsd at which the same extent fits.
inline int frame_check(const float c[3], const float a[3], const float e[3], const float b[3], float radius, float gsd, int64_t w,
                       int64_t h, float d_min, float d_max, int32_t side, const char **why, double *fit_gsd) {
  *fit_gsd = 0.0;
  auto refuse = [&](const char *what, int code) {
    *why = what;
    return code;
  };
  bool finite = std::isfinite(gsd) && std::isfinite(d_min) && std::isfinite(d_max) && std::isfinite(radius);
  for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(c[k]) && std::isfinite(a[k]) && std::isfinite(e[k]) && std::isfinite(b[k]);
  if (!finite) return refuse("a value of the frame is not finite", 1);
  if (!(gsd >= 1e-4f && gsd <= 1.0f)) return refuse("gsd outside [1e-4, 1]", 1);
  if (!(radius >= kMinRadius && radius <= kMaxRadius)) return refuse("radius outside [0.05, 1000]", 1);
  if (side != 1 && side != -1) return refuse("side is +1 (seen from inside) or -1 (seen from outside)", 1);
  if (!(d_min < d_max)) return refuse("the depth window is empty (d_min < d_max is required)", 1);
  if (w < 1 || h < 1) return refuse("width and height start at 1", 1);
  const double E[3] = {e[0], e[1], e[2]}, B[3] = {b[0], b[1], b[2]}, A[3] = {a[0], a[1], a[2]};
  auto dot = [](const double *p, const double *q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
  const double cross[3] = {E[1] * B[2] - E[2] * B[1], E[2] * B[0] - E[0] * B[2], E[0] * B[1] - E[1] * B[0]};
  const double tol = 1e-3;
  bool ok = std::fabs(dot(E, E) - 1.0) <= tol && std::fabs(dot(B, B) - 1.0) <= tol && std::fabs(dot(A, A) - 1.0) <= tol &&
            std::fabs(dot(E, B)) <= tol && std::fabs(dot(E, A)) <= tol && std::fabs(dot(B, A)) <= tol;
  for (int k = 0; k < 3; ++k) ok = ok && std::fabs(cross[k] - static_cast<double>(side) * A[k]) <= tol;
  if (!ok) return refuse("the axes are not orthonormal with e x b = side a within 1e-3", 1);
  if (static_cast<double>(w) * static_cast<double>(gsd) > kTwoPi * static_cast<double>(radius) + static_cast<double>(gsd))
    return refuse("the raster is wider than the circumference (width gsd <= 2 pi R + gsd is required)", 1);
  if (w > om::kMaxSide || h > om::kMaxSide || w * h > om::kMaxPixels) {
    *fit_gsd = om::fit_gsd(static_cast<double>(w) * gsd, static_cast<double>(h) * gsd, 0.0);
    return refuse("the raster exceeds 16384 a side or 2^26 pixels", 2);
  }
  return 0;
}

}  // namespace cy
}  // namespace pcp
