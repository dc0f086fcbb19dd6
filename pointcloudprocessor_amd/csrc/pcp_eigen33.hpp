// pcp_eigen33.hpp -- pcl::eigen33's smallest eigenpair in closed form and the two fp64 reciprocals it rests on, for the
// kernels that fit a plane to a neighbourhood: the MLS fit (pcp_mls.hip), the map normals (pcp_normals.hip), the crack-width
// plane (pcp_crack_width.hip) and the crack tangent (pcp_crack_direction.hip).  Device only.  Floating-point contraction is
// the includer's: pcp_mls.hip allows it (tolerance-gated stage), the other three are built without.
// pcp_selftest_eigen33 (pcp_eigen33_selftest.hpp) runs these functions on a caller's input in both compilations;
// tests/test_eigen33_gpu.py holds them to mpmath at 50 digits, tests/_eigen33_ref.py is the plain fp64 restatement.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace pcp {

// 1 / x and 1 / sqrt(x) in fp64 to an ulp or two: the hardware estimate and Newton steps, without the range scaling, the exact
// residual correction and the special-case fix-ups of the IEEE sequences (~8 instead of ~28 instructions).  For the fit's own
// arithmetic (tolerance-gated against the oracle: 3 um, 1e-4), whose operands are covariances, lengths and pivots -- normal
// numbers; zero, negative and non-finite arguments give infinities / NaNs that the callers' guards (ok, isfinite) catch as before.
// Measured on 2^k (1 + f), k in [-1000, 1000] (10^6 arguments, both signs for 1 / x): mls_rcp returned the correctly rounded
// value every time, mls_rsqrt is within 1 ulp of it (the test's bar is the 2 ulp claimed here).
__device__ __forceinline__ double mls_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = __builtin_fma(-x, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-x, r, 1.0);
  return __builtin_fma(r, e, r);
}
__device__ __forceinline__ double mls_rsqrt(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  const double e = __builtin_fma(-(x * y), y, 1.0);
  return __builtin_fma(y * e, __builtin_fma(0.375, e, 0.5), y);
}

// ---- pcl::eigen33 smallest eigenpair (common/impl/eigen.hpp) [upstream] --------
__device__ __forceinline__ void roots2(double b, double c, double &r0, double &r1, double &r2) {
  r0 = 0.0;
  double d = b * b - 4.0 * c;
  if (d < 0.0) d = 0.0;
  const double sd = sqrt(d);
  r2 = 0.5 * (b + sd);
  r1 = 0.5 * (b - sd);
}

__device__ __forceinline__ void swap2(double &a, double &b) {
  const double t = a;
  a = b;
  b = t;
}

// the longest cross product of two rows of A - r0 I counts as a direction above this multiple of the squared largest entry
constexpr double kCrossNoise = 256.0 * DBL_EPSILON;

// (inlined: as a call it cost the kernel 96 bytes of scratch per lane and a save / restore around it -- fit 4.25 -> 4.12 ms)
__device__ __forceinline__ void smallest_eigenpair(const double m[6] /* xx xy xz yy yz zz */, double &ev, double n[3]) {
  double scale = fmax(fmax(fmax(fabs(m[0]), fabs(m[1])), fmax(fabs(m[2]), fabs(m[3]))), fmax(fabs(m[4]), fabs(m[5])));
  if (scale <= DBL_MIN) scale = 1.0;
  const double inv_scale = mls_rcp(scale);
  const double a00 = m[0] * inv_scale, a01 = m[1] * inv_scale, a02 = m[2] * inv_scale, a11 = m[3] * inv_scale,
               a12 = m[4] * inv_scale, a22 = m[5] * inv_scale;
  const double c0 = a00 * a11 * a22 + 2.0 * a01 * a02 * a12 - a00 * a12 * a12 - a11 * a02 * a02 - a22 * a01 * a01;
  const double c1 = a00 * a11 - a01 * a01 + a00 * a22 - a02 * a02 + a11 * a22 - a12 * a12;
  const double c2 = a00 + a11 + a22;
  double r0, r1, r2;
  if (fabs(c0) < DBL_EPSILON) {
    roots2(c2, c1, r0, r1, r2);
  } else {
    const double inv3 = 1.0 / 3.0;
    const double sqrt3 = sqrt(3.0);
    const double c2_3 = c2 * inv3;
    double a_3 = (c1 - c2 * c2_3) * inv3;
    if (a_3 > 0.0) a_3 = 0.0;
    const double half_b = 0.5 * (c0 + c2_3 * (2.0 * c2_3 * c2_3 - c1));
    double q = half_b * half_b + a_3 * a_3 * a_3;
    if (q > 0.0) q = 0.0;
    const double rho = sqrt(-a_3);
    const double theta = atan2(sqrt(-q), half_b) * inv3;
    const double ct = cos(theta), st = sin(theta);
    r0 = c2_3 + 2.0 * rho * ct;
    r1 = c2_3 - rho * (ct + sqrt3 * st);
    r2 = c2_3 - rho * (ct - sqrt3 * st);
    if (r0 >= r1) swap2(r0, r1);
    if (r1 >= r2) {
      swap2(r1, r2);
      if (r0 >= r1) swap2(r0, r1);
    }
    if (r0 <= 0.0) roots2(c2, c1, r0, r1, r2);
  }
  ev = r0 * scale;
  // getLargest3x3Eigenvector of (A - r0 I): longest cross product of two rows
  const double s00 = a00 - r0, s11 = a11 - r0, s22 = a22 - r0;
  const double k0x = a01 * a12 - a02 * s11, k0y = a02 * a01 - s00 * a12, k0z = s00 * s11 - a01 * a01;  // row0 x row1
  const double k1x = a01 * s22 - a02 * a12, k1y = a02 * a02 - s00 * s22, k1z = s00 * a12 - a01 * a02;  // row0 x row2
  const double k2x = s11 * s22 - a12 * a12, k2y = a12 * a02 - a01 * s22, k2z = a01 * a12 - s11 * a02;  // row1 x row2
  const double l0 = (k0x * k0x + k0y * k0y) + k0z * k0z;
  const double l1 = (k1x * k1x + k1y * k1y) + k1z * k1z;
  const double l2 = (k2x * k2x + k2y * k2y) + k2z * k2z;
  double vx = k0x, vy = k0y, vz = k0z, l = l0;
  if (l1 > l) {
    vx = k1x; vy = k1y; vz = k1z; l = l1;
  }
  if (l2 > l) {
    vx = k2x; vy = k2y; vz = k2z; l = l2;
  }
  // A cross product at the rounding of its own terms is no direction.  Each component is a difference of two products of
  // entries of A - r0 I, which carry the error of r0 (a few ulp of the trace) and their own roundings: below ~50 ulp of the
  // squared largest entry the longest cross product is noise, and its unit vector need not lie anywhere near the null space
  // (a neighbourhood of two distinct positions, an exact needle l0 = l1: residual |A n - ev n| / l2 of order 1, reported as a
  // valid normal; tests/test_eigen33_cpu.py, profiles/eigen33_selftest.md).  Such a vector is NaN like that of l == 0, which
  // the callers' guards (isfinite) already catch.  Where a plane is defined the ratio is above 1e-5 -- (l1 - l0) / l2 of the
  // neighbourhood, within a factor of 9 -- and nothing changes; quantised lines (1e-11 and more) keep their normal too.
  double big = fmax(fmax(fmax(fabs(s00), fabs(s11)), fmax(fabs(s22), fabs(a01))), fmax(fabs(a02), fabs(a12)));
  big *= big;
  const double inv_len = l > (kCrossNoise * kCrossNoise) * (big * big) ? mls_rsqrt(l) : NAN;  // (l == 0 and l NaN: NaN as before)
  n[0] = vx * inv_len;
  n[1] = vy * inv_len;
  n[2] = vz * inv_len;
}

}  // namespace pcp
