// pcp_visit_forms.hpp -- three pieces of a (tile, keyframe) visit of the batched passes, each in the form the reference writes
// ("written") and in a shorter form that returns the same bits ("short"), for host and device from the same text.  The kernels
// (pcp_device.hpp) run the short forms; pcp_selftest_visit_forms() runs both side by side on the device and
// host/visit_forms_selftest.cpp does in plain C++.  Every identity below is exact: there is no error bound and no fallback for
// precision, only a guard where the identity needs its operands in a range.
// Build with -ffp-contract=off: every multiply and add is individually rounded, every fused operation is an explicit FMA.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PCP_VF_HD __host__ __device__ __forceinline__
#define PCP_VF_FMA(a, b, c) __builtin_fma((a), (b), (c))
#define PCP_VF_FMAF(a, b, c) __builtin_fmaf((a), (b), (c))
#define PCP_VF_FMINF(a, b) __builtin_fminf((a), (b))
#else
#include <cmath>
#define PCP_VF_HD inline
#define PCP_VF_FMA(a, b, c) std::fma((a), (b), (c))
#define PCP_VF_FMAF(a, b, c) std::fma((a), (b), (c))
#define PCP_VF_FMINF(a, b) std::fmin((a), (b))
#endif

namespace pcp {
namespace vf {

// ---- 1. distortion (pinhole.hpp:19-33): normalised (xn, yn) -> distorted (xd, yd), fp64 -----------------------------------
struct Distortion {
  double k1, k2, k3, p1, p2;
};

// left to right as the reference writes it
PCP_VF_HD void distort_written(const Distortion &c, double xn, double yn, double &xd, double &yd) {
  const double x2 = xn * xn;
  const double y2 = yn * yn;
  const double r2 = x2 + y2;
  const double r4 = r2 * r2;
  const double r6 = r2 * r4;
  const double rc = ((1.0 + c.k1 * r2) + c.k2 * r4) + c.k3 * r6;
  const double t1 = (2.0 * xn) * yn;
  const double t2 = r2 + 2.0 * x2;
  const double t3 = r2 + 2.0 * y2;
  xd = (rc * xn + c.p1 * t1) + c.p2 * t2;
  yd = (rc * yn + c.p1 * t3) + c.p2 * t1;
}

// Three instructions fewer: the doublings are folded into FMAs.  Doubling is exact unless it overflows, and
// RN(2 a) = 2 RN(a) unless RN(a) is subnormal, so with w = RN(xn yn), a = RN(p1 w), b = RN(p2 w):
//   t1 = RN(RN(2 xn) yn) = 2 w          p1 t1 -> RN(p1 2 w) = 2 a          p2 t1 -> 2 b
//   t2 = RN(r2 + RN(2 x2)) = RN(r2 + 2 x2) = fma(2, x2, r2), t3 likewise
//   RN(RN(rc xn) + 2 a) = fma(2, a, RN(rc xn))         RN(S + 2 b) = fma(2, b, S),  S = RN(RN(rc yn) + RN(p1 t3))
// Ranges: xn, yn are correctly rounded quotients of promoted floats, so each is 0, non-finite, or 2^-277 <= |.| <= 2^277:
// 2 xn, 2 x2, 2 y2 and 2 w cannot overflow, and x2, y2, w are 0 or >= 2^-554, never subnormal.  a and b are 0 or within
// [2^-954, 2^954] when every non-zero |p1|, |p2| lies in [2^-400, 2^400] -- distortion_is_tame(), which pcp_set_camera turns
// into pcp_context::uv_tame; other coefficients keep the written form.
// Zeros: 2 (+-0) = +-0 and w, a, b carry the signs of t1 / 2, p1 t1 / 2, p2 t1 / 2; an FMA whose exact result is 0 returns the
// zero the written addition of the same two terms returns.  Non-finite values: doubling maps inf to inf and NaN to NaN, so every
// operation below sees an infinity or a NaN exactly where the written one does and produces the same class (inf - inf and
// 0 inf are NaN in both); NaN payloads are not observable (every later use is a comparison).
PCP_VF_HD void distort_short(const Distortion &c, double xn, double yn, double &xd, double &yd) {
  const double x2 = xn * xn;
  const double y2 = yn * yn;
  const double r2 = x2 + y2;
  const double r4 = r2 * r2;
  const double r6 = r2 * r4;
  const double rc = ((1.0 + c.k1 * r2) + c.k2 * r4) + c.k3 * r6;
  const double w = xn * yn;
  const double a = c.p1 * w, b = c.p2 * w;
  const double t2 = PCP_VF_FMA(2.0, x2, r2);
  const double t3 = PCP_VF_FMA(2.0, y2, r2);
  xd = PCP_VF_FMA(2.0, a, rc * xn) + c.p2 * t2;
  yd = PCP_VF_FMA(2.0, b, rc * yn + c.p1 * t3);
}

PCP_VF_HD bool tame_coefficient(double p) {
  const double m = p < 0.0 ? -p : p;
  return p == 0.0 || (m >= 0x1p-400 && m <= 0x1p400);  // NaN: false
}
PCP_VF_HD bool distortion_is_tame(double p1, double p2) { return tame_coefficient(p1) && tame_coefficient(p2); }

// ---- 2. cell of the depth map from the two fp32 quotients (view_culling.cpp:86-90, :116, :155), depth buffer on -------------
// written: each axis against the FULL cull size (sic), C truncation, then against the map (mw = cull_w / ds, mh likewise).
// Returns cy * mw + cx or -1.  (0 <= (int)q < W  <=>  -1 < q < W for an integer W below 2^24; NaN / inf / out-of-int32 fail.)
PCP_VF_HD int32_t map_cell_written(float qx, float qy, float cull_wf, float cull_hf, int32_t mw, int32_t mh) {
  const int32_t cx = ((qx > -1.0f) & (qx < cull_wf)) ? static_cast<int32_t>(qx) : -1;
  const int32_t cy = ((qy > -1.0f) & (qy < cull_hf)) ? static_cast<int32_t>(qy) : -1;
  if ((cx < 0) | (cy < 0)) return -1;
  return ((cx < mw) & (cy < mh)) ? cy * mw + cx : -1;
}

// the bound the short form compares a quotient with: the map size as fp32 (exact: below 2^24); an empty map (cull size below
// ds) gets -1, which no q > -1 is below -- with W = 0 a quotient in (-1, 0) truncates to 0, which is not < 0, but is < 0.0f
PCP_VF_HD float map_bound(int32_t cells_along_axis) { return cells_along_axis > 0 ? static_cast<float>(cells_along_axis) : -1.0f; }

// short: ds >= 1 gives mw <= cull_w, so q < mw implies the test against the cull size, and for q > -1 and mw >= 1,
// (int)q < mw  <=>  q < mw (q in (-1, 0) truncates to 0 < mw; q >= 0: trunc(q) < mw <=> q < mw, mw an integer).
// The two lower bounds share one comparison, fmin(qx, qy) > -1: a NaN that the minimum drops fails its own upper bound.
// A minimum, three compares, two conversions, one multiply-add.  `cell` is only meaningful when the result is true.
PCP_VF_HD bool map_cell_short(float qx, float qy, float mwf, float mhf, int32_t mw, int32_t &cell) {
  const float lo = PCP_VF_FMINF(qx, qy);
  const bool ok = (lo > -1.0f) & (qx < mwf) & (qy < mhf);
  cell = ok ? static_cast<int32_t>(qy) * mw + static_cast<int32_t>(qx) : 0;
  return ok;
}

// ---- 4. RN(sqrt(x)) in fp32 from an estimate within 1 ulp (computeDistanceScore, hpp:222-236) -------------------------------
// The correctly rounded square root is the estimate s or one of its two neighbours: with d = pred(s), u = succ(s) (bit pattern
// -+ 1), the residuals x - d s and x - u s by FMA are exact enough in sign to decide (the scheme the compiler emits between its
// range scaling and its class test): x <= d s -> d; x > u s -> u; else s.  In the window below nothing under- or overflows:
// s >= 2^-48 with an ulp of at least 2^-71, so the products are >= 2^-97 and the exact residuals multiples of 2^-142, which the
// FMA cannot round to zero or to the other sign.
// (the window as one unsigned comparison of the bit pattern: 0x0f800000 is 2^-96, 0x7f800000 the first pattern above FLT_MAX;
// negative numbers and NaNs wrap or stay above)
PCP_VF_HD bool sqrt_in_window(float x) {
  union {
    float f;
    uint32_t u;
  } b;
  b.f = x;
  return b.u - 0x0f800000u < 0x7f800000u - 0x0f800000u;
}

PCP_VF_HD float sqrt_from_estimate(float x, float s) {
  union {
    float f;
    uint32_t u;
  } b;
  b.f = s;
  const uint32_t sb = b.u;
  b.u = sb - 1u;
  const float dn = b.f;
  b.u = sb + 1u;
  const float up = b.f;
  const float vp = PCP_VF_FMAF(-dn, s, x);
  const float vs = PCP_VF_FMAF(-up, s, x);
  float r = vp <= 0.0f ? dn : s;
  r = vs > 0.0f ? up : r;
  return r;
}

}  // namespace vf
}  // namespace pcp
