// pcp_tile_classify.hpp -- the conservative verdict on a bounding sphere against one keyframe, shared by the tile masks of the
// colour path (pcp_colour.hip, K0: tile_classify_box, the sphere and the tile's box) and the keyframe lists of the orthophoto's
// tiles (pcp_ortho_texture.hip, OT7: tile_classify).
//
// A (sphere, keyframe) pair is REJECTED only when every point inside the sphere is certain to be rejected by the reference
// in that keyframe, proved in fp64 with outward-padded interval arithmetic:
//   (a) the sphere, transformed with the fp32 matrix the reference uses and
//       inflated by the matrix's spectral-norm bound and the fp32 rounding slack of
//       the per-point transform, lies in z <= 0; or
//   (b) it lies in z > 0 and the interval image of its normalised coordinates under
//       the distortion polynomial misses the acceptance box of both the cull-cell
//       and the colour-pixel rule (same box as surely_rejected()).
// Anything else (straddling z = 0, fold-back distortion, huge spheres) is kept.
#pragma once

#include "pcp_device.hpp"
#include "pcp_tile_box.hpp"

namespace pcp {

struct Interval {
  double lo, hi;
};
__device__ __forceinline__ Interval iv_add(Interval a, Interval b) { return {a.lo + b.lo, a.hi + b.hi}; }
__device__ __forceinline__ Interval iv_scale(double k, Interval a) {
  return k >= 0.0 ? Interval{k * a.lo, k * a.hi} : Interval{k * a.hi, k * a.lo};
}
__device__ __forceinline__ Interval iv_mul(Interval a, Interval b) {
  const double p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
  return {fmin(fmin(p0, p1), fmin(p2, p3)), fmax(fmax(p0, p1), fmax(p2, p3))};
}
__device__ __forceinline__ Interval iv_sqr(Interval a) {
  const double l = fabs(a.lo), h = fabs(a.hi);
  const double mx = fmax(l, h), mn = (a.lo <= 0.0 && a.hi >= 0.0) ? 0.0 : fmin(l, h);
  return {mn * mn, mx * mx};
}
// a >= 0 and b >= 0 (squares, and reciprocals of positive numbers): the corner products are the bounds
__device__ __forceinline__ Interval iv_mul_pos(Interval a, Interval b) { return {a.lo * b.lo, a.hi * b.hi}; }
// b > 0: the sign of each bound of a picks its factor
__device__ __forceinline__ Interval iv_mul_by_pos(Interval a, Interval b) {
  return {a.lo * (a.lo >= 0.0 ? b.lo : b.hi), a.hi * (a.hi >= 0.0 ? b.hi : b.lo)};
}
// 1 / x of a positive normal x, within 1e-14 relative (the hardware estimate and two Newton steps; the intervals are padded by
// 1e-12 wherever it is used: an exactly rounded quotient costs three times the instructions)
__device__ __forceinline__ double iv_rcp_pos(double b) {
  double r = __builtin_amdgcn_rcp(b);
  r = fma(fma(-b, r, 1.0), r, r);
  r = fma(fma(-b, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ Interval iv_pad(Interval a) {  // absorbs the fp64 rounding of the interval arithmetic
  const double e = 1e-12 * (fabs(a.lo) + fabs(a.hi)) + 1e-300;
  return {a.lo - e, a.hi + e};
}

// Returns 1 when every point of the tile is certain to be rejected (exactness-critical, see above),
// 2 when the whole tile images strictly inside the acceptance box (a performance hint only: the
// per-point fp32 rejection test could not reject anything there, so the depth pass skips it), else 0.
__device__ __forceinline__ int tile_classify(const DevCamera &c, const DevFrame &fr, float4 sph) {
  const double cx = sph.x, cy = sph.y, cz = sph.z;
  const float *m = fr.w2c;
  const double X = (m[0] * cx + m[1] * cy) + (m[2] * cz + m[3]);
  const double Y = (m[4] * cx + m[5] * cy) + (m[6] * cz + m[7]);
  const double Z = (m[8] * cx + m[9] * cy) + (m[10] * cz + m[11]);
  // |M (p - c)| <= s |p - c|; fp32 transform rounding <= 3 * 2^-24 * sum of term magnitudes
  const double mag = fr.norm_bound * (fabs(cx) + fabs(cy) + fabs(cz) + 3.0 * sph.w) + fabs(static_cast<double>(m[3])) +
                     fabs(static_cast<double>(m[7])) + fabs(static_cast<double>(m[11])) + 1e-3;
  const double rho = fr.norm_bound * static_cast<double>(sph.w) * (1.0 + 1e-6) + 1e-6 * mag;
  if (!(rho >= 0.0) || !isfinite(X + Y + Z + rho)) return 0;
  if (Z + rho <= 0.0) return 1;   // (a) entirely behind the camera
  if (Z - rho <= 0.0) return 0;  // straddles z = 0: no bound on x / z
  const Interval zi{Z - rho, Z + rho};
  if (!(zi.lo >= 1e-290)) return 0;  // (a subnormal depth: no reciprocal estimate, no verdict)
  const Interval iz{iv_rcp_pos(zi.hi) * (1.0 - 1e-13), iv_rcp_pos(zi.lo) * (1.0 + 1e-13)};
  const Interval xn = iv_pad(iv_mul_by_pos(Interval{X - rho, X + rho}, iz));
  const Interval yn = iv_pad(iv_mul_by_pos(Interval{Y - rho, Y + rho}, iz));
  const Interval x2 = iv_sqr(xn), y2 = iv_sqr(yn);
  const Interval r2 = iv_add(x2, y2);
  const Interval r4 = iv_mul_pos(r2, r2);
  const Interval r6 = iv_mul_pos(r2, r4);
  Interval rc = iv_add(iv_add(iv_scale(c.k1, r2), iv_scale(c.k2, r4)), iv_scale(c.k3, r6));
  rc.lo += 1.0;
  rc.hi += 1.0;
  const Interval t1 = iv_scale(2.0, iv_mul(xn, yn));
  const Interval t2 = iv_add(r2, iv_scale(2.0, x2));
  const Interval t3 = iv_add(r2, iv_scale(2.0, y2));
  const Interval xd = iv_pad(iv_add(iv_add(iv_mul(rc, xn), iv_scale(c.p1, t1)), iv_scale(c.p2, t2)));
  const Interval yd = iv_pad(iv_add(iv_add(iv_mul(rc, yn), iv_scale(c.p1, t3)), iv_scale(c.p2, t1)));
  Interval u = iv_pad(iv_scale(c.fx, xd)), v = iv_pad(iv_scale(c.fy, yd));
  u.lo += c.cx; u.hi += c.cx;
  v.lo += c.cy; v.hi += c.cy;
  if (!isfinite(u.lo + u.hi + v.lo + v.hi)) return 0;
  // the box already carries a 0.5 px margin (pcp_set_camera)
  if (u.hi < static_cast<double>(c.u_lo) || u.lo > static_cast<double>(c.u_hi) ||
      v.hi < static_cast<double>(c.v_lo) || v.lo > static_cast<double>(c.v_hi))
    return 1;
  return (u.lo > static_cast<double>(c.u_lo) + 1.0 && u.hi < static_cast<double>(c.u_hi) - 1.0 &&
          v.lo > static_cast<double>(c.v_lo) + 1.0 && v.hi < static_cast<double>(c.v_hi) - 1.0)
             ? 2
             : 0;
}

// The same verdict on a tile that also knows the half-extents h of its world-axis box about the sphere's centre (the tiles
// and groups of an uploaded cloud, pcp_context.hip k_up_bounds).  The only difference from tile_classify is the inflation of the
// three camera coordinates, one per row r of the matrix instead of one for all (pcp_tile_box.hpp tile_inflation, with the
// soundness argument):
//   rho_r = min(rho, (sum_j |m_rj| h_j) (1 + 1e-6) + 1e-6 mag),   rho and mag as above,
// because |(M (p - c))_r| <= sum_j |m_rj| |p_j - c_j| <= sum_j |m_rj| h_j for every member p, and the sphere's bound holds for
// every row as before.  The intervals are X +- rho_0, Y +- rho_1, Z +- rho_2; both z tests and the reciprocal use rho_2.  From
// there on the interval image is tile_classify's, so the verdicts keep their meaning: 2 still says that every point of the tile
// images inside the box, and the group-level shortcut of the mask kernels stays valid.
// (tile_classify keeps its text: pcp_ortho_texture.hip calls it with spheres of its own.)
__device__ __forceinline__ int tile_classify_box(const DevCamera &c, const DevFrame &fr, float4 sph, float4 ext) {
  const double cx = sph.x, cy = sph.y, cz = sph.z;
  const float *m = fr.w2c;
  const double X = (m[0] * cx + m[1] * cy) + (m[2] * cz + m[3]);
  const double Y = (m[4] * cx + m[5] * cy) + (m[6] * cz + m[7]);
  const double Z = (m[8] * cx + m[9] * cy) + (m[10] * cz + m[11]);
  const TileInflation inf = tile_inflation(m, fr.norm_bound, cx, cy, cz, sph.w, ext.x, ext.y, ext.z);
  const double rho = inf.sphere, rx = inf.row[0], ry = inf.row[1], rz = inf.row[2];
  if (!(rho >= 0.0) || !isfinite(X + Y + Z + rho)) return 0;
  if (Z + rz <= 0.0) return 1;   // (a) entirely behind the camera
  if (Z - rz <= 0.0) return 0;  // straddles z = 0: no bound on x / z
  const Interval zi{Z - rz, Z + rz};
  if (!(zi.lo >= 1e-290)) return 0;  // (a subnormal depth: no reciprocal estimate, no verdict)
  const Interval iz{iv_rcp_pos(zi.hi) * (1.0 - 1e-13), iv_rcp_pos(zi.lo) * (1.0 + 1e-13)};
  const Interval xn = iv_pad(iv_mul_by_pos(Interval{X - rx, X + rx}, iz));
  const Interval yn = iv_pad(iv_mul_by_pos(Interval{Y - ry, Y + ry}, iz));
  const Interval x2 = iv_sqr(xn), y2 = iv_sqr(yn);
  const Interval r2 = iv_add(x2, y2);
  const Interval r4 = iv_mul_pos(r2, r2);
  const Interval r6 = iv_mul_pos(r2, r4);
  Interval rc = iv_add(iv_add(iv_scale(c.k1, r2), iv_scale(c.k2, r4)), iv_scale(c.k3, r6));
  rc.lo += 1.0;
  rc.hi += 1.0;
  const Interval t1 = iv_scale(2.0, iv_mul(xn, yn));
  const Interval t2 = iv_add(r2, iv_scale(2.0, x2));
  const Interval t3 = iv_add(r2, iv_scale(2.0, y2));
  const Interval xd = iv_pad(iv_add(iv_add(iv_mul(rc, xn), iv_scale(c.p1, t1)), iv_scale(c.p2, t2)));
  const Interval yd = iv_pad(iv_add(iv_add(iv_mul(rc, yn), iv_scale(c.p1, t3)), iv_scale(c.p2, t1)));
  Interval u = iv_pad(iv_scale(c.fx, xd)), v = iv_pad(iv_scale(c.fy, yd));
  u.lo += c.cx; u.hi += c.cx;
  v.lo += c.cy; v.hi += c.cy;
  if (!isfinite(u.lo + u.hi + v.lo + v.hi)) return 0;
  if (u.hi < static_cast<double>(c.u_lo) || u.lo > static_cast<double>(c.u_hi) ||
      v.hi < static_cast<double>(c.v_lo) || v.lo > static_cast<double>(c.v_hi))
    return 1;
  return (u.lo > static_cast<double>(c.u_lo) + 1.0 && u.hi < static_cast<double>(c.u_hi) - 1.0 &&
          v.lo > static_cast<double>(c.v_lo) + 1.0 && v.hi < static_cast<double>(c.v_hi) - 1.0)
             ? 2
             : 0;
}

}  // namespace pcp
