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
//
// kK3 = false: without the k3 term -- r6, k3 r6 and the last addition of rc, three instructions -- for a camera whose k3 is a zero
// (the reference's own constants, every camera of synth.py) and whose other constants pass k3_term_droppable() below, which
// pcp_set_camera turns into pcp_context::k3_dropped; any other camera keeps the term.  The lane's VERDICTS are the same -- u and v
// bit for bit wherever the written form accepts a lane, and a rejection by both truncation rules wherever it rejects one.
// With S = RN(RN(1 + k1 r2) + RN(k2 r4)), the rc of this form, and k3 = +-0:
//   a. r6 finite: k3 r6 = +-0 and S + (+-0) = S unless S = -0, which it never is: a sum is -0 only when both terms are, and
//      RN(1 + t) is not (1 is not -0; an exact 0 rounds to +0).  S infinite or NaN: unchanged by the addition.  Same bits.
//   b. r2 NaN (xn or yn NaN, or inf - inf on the way): rc is NaN in both forms.
//   c. r6 = inf.  The written form has k3 r6 = 0 inf = NaN, so u and v are NaN and both rules reject the lane; this form must
//      reject it too.  r6 = inf needs r2^3 >= 2^1024 (1 - 2^-54), r2 >= 2^341.3, so M = max(|xn|, |yn|) >= 2^170 (r2 <= 2 M^2 (1 +
//      2^-52)), or xn / yn infinite.  If S is not finite (r2 or r4 infinite -- k2 inf is +-inf, 0 inf NaN -- or the sum overflowed),
//      rc xn and rc yn are infinite or NaN, and an infinity or a NaN stays one through every later multiply, add and FMA (inf 0 and
//      inf - inf are NaN): u and v are not finite, rejected.  Else every value below is finite, M <= 2^277 (see the ranges above), and
//      say |xn| = M (for |yn| = M read yd, b, p1 t3, fy, cy).  Under k3_term_droppable() -- k1, k2, p1, p2 each 0 or of
//      magnitude in [2^-60, 2^60], |fx|, |fy| in [2^-20, 2^40], |cx|, |cy| <= 2^40 -- and with every operation's relative
//      error below 2^-52 (nothing here is near the subnormal range):
//        k2 != 0:          |k2 r4| >= 2^-61 M^4 against |1 + k1 r2| <= 2^62 M^2, a factor 2^-123 M^2 >= 2^217:  |S| >= 2^-62 M^4
//        k2 = 0, k1 != 0:  k2 r4 = +-0, |k1 r2| >= 2^-61 M^2 against 1:                                          |S| >= 2^-62 M^2
//        k1 = k2 = 0:      S = 1, and the condition then asks for p1 = p2 = 0: a = b = +-0, p2 t2 = +-0, xd = xn exactly
//      In the first two |S xn| >= 2^-63 M^3 (or it overflows: see above) against |2 a| <= 2^62 M^2 and |p2 t2| <= 2^63 M^2
//      (t2 <= 4 M^2 (1 + 2^-51)), together below 2^64 M^2: smaller by 2^-127 M >= 2^43, so |xd| >= 2^-64 M^3 >= 2^446; in the third
//      |xd| = M >= 2^170.  Then |fx xd| >= 2^150 against |cx| <= 2^40: |u| >= 2^149 or infinite, outside every image and, as fp32
//      an infinity, outside every map (div_by_ds, cell_of_quotient).  Rejected by both rules on the strength of u alone.
// (k1 = k2 = 0 with a tangential term is left out: xd = xn (1 + 2 p1 yn) + p2 t2 can cancel.  Such a camera keeps the term.)
template <bool kK3 = true>
PCP_VF_HD void distort_short(const Distortion &c, double xn, double yn, double &xd, double &yd) {
  const double x2 = xn * xn;
  const double y2 = yn * yn;
  const double r2 = x2 + y2;
  const double r4 = r2 * r2;
  const double r6 = r2 * r4;  // (unused without the term)
  const double rc = kK3 ? ((1.0 + c.k1 * r2) + c.k2 * r4) + c.k3 * r6 : (1.0 + c.k1 * r2) + c.k2 * r4;
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

// the condition of distort_short<false> (case c of its proof); NaNs fail every comparison
PCP_VF_HD bool magnitude_within(double p, double lo, double hi) {
  const double m = p < 0.0 ? -p : p;
  return m >= lo && m <= hi;
}
PCP_VF_HD bool k3_term_droppable(const Distortion &c, double fx, double fy, double cx, double cy) {
  const bool zero_or_mid[4] = {c.k1 == 0.0 || magnitude_within(c.k1, 0x1p-60, 0x1p60), c.k2 == 0.0 || magnitude_within(c.k2, 0x1p-60, 0x1p60),
                               c.p1 == 0.0 || magnitude_within(c.p1, 0x1p-60, 0x1p60), c.p2 == 0.0 || magnitude_within(c.p2, 0x1p-60, 0x1p60)};
  const bool radial = c.k1 != 0.0 || c.k2 != 0.0;       // a leading coefficient, or ...
  const bool plain = c.p1 == 0.0 && c.p2 == 0.0;        // ... no distortion at all
  return c.k3 == 0.0 && zero_or_mid[0] && zero_or_mid[1] && zero_or_mid[2] && zero_or_mid[3] && (radial || plain) &&
         magnitude_within(fx, 0x1p-20, 0x1p40) && magnitude_within(fy, 0x1p-20, 0x1p40) && magnitude_within(cx, 0.0, 0x1p40) &&
         magnitude_within(cy, 0.0, 0x1p40);
}

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
