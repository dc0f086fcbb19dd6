// pcp_crack_width.hpp -- the per-element arithmetic of the crack width maps ("Crack width maps", CW1-CW9), one
// copy for the kernels (pcp_crack_width.hip), the CPU form (pcp_crack_width_host) and the host self-test
// (host/crack_width_selftest.cpp): the ridge test, the integer trace, the quantisation and the recentred moments of the
// plane window, the undistortion of an edge point and the ray-plane intersection.  Every integer result is exact; the moments
// are taken modulo 2^64 in unsigned arithmetic and are exact because the true values fit.  Build without floating-point
// contraction: every fp64 operation below is rounded on its own.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define PCP_CW_HD __host__ __device__ __forceinline__
#else
#define PCP_CW_HD inline
#endif

namespace pcp {
namespace cw {

// CW9: the flag byte
constexpr uint8_t kSite = 1, kCentre = 2, kNear = 4, kFar = 8, kPlane = 16, kRays = 32, kWidth = 64;
constexpr int32_t kMinRadius = 1, kMaxRadius = 181;   // CW4: (2 * 181)^2 < 2^17 members at most
constexpr int32_t kMaxSide = 16384;                   // CW3: every intermediate of the trace fits int32
constexpr int64_t kMaxPixels = int64_t(1) << 26;      // W * H of one call
constexpr float kQuantaPerMetre = 65536.0f;           // CW4: 2^16, the quantum is ~15 um
constexpr float kMaxCoordinate = 64.0f;               // CW4: |xyz_cam| below this on all three axes, so |q| <= 2^22
constexpr int32_t kMinMembers = 3;                    // CW6
constexpr int kOriginPlanes = 10;                     // n S1x S1y S1z S2xx xy xz yy yz zz about the camera origin
constexpr int kMomentWords = 13;                      // n r[3] S1'[3] S2'[6]
constexpr int kUndistortSteps = 10;                   // CW7
constexpr double kReprojectionPx = 1e-3;              // CW7: the redistorted ray must come back this close on both axes
constexpr double kMinIncidence = 0.1;                 // CW7: |n . d| >= 0.1 |d|
constexpr uint32_t kSentinelD2 = 0xffffffffu;         // MD5: the mask has no background pixel

PCP_CW_HD bool radius_ok(int32_t r) { return r >= kMinRadius && r <= kMaxRadius; }

// ---- CW2: the ridge of the distance transform --------------------------------------------------------------------------
// d2(x, y) for pixels inside the image
template <typename D2>
PCP_CW_HD bool is_centre(const D2 &d2, int32_t x, int32_t y, int32_t w, int32_t h) {
  const uint32_t mine = d2(x, y);
  for (int32_t dy = -1; dy <= 1; ++dy)
    for (int32_t dx = -1; dx <= 1; ++dx) {
      const int32_t qx = x + dx, qy = y + dy;
      if ((dx | dy) == 0 || qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
      if (d2(qx, qy) > mine) return false;
    }
  return true;
}

// ---- CW3: the trace -------------------------------------------------------------------------------------------------------
// rdiv(n, a) = (2n + a) div (2a), n >= 0, a > 0: n / a rounded to nearest, halves up.  rdiv(a * m, a) = m.
PCP_CW_HD int32_t rdiv(int32_t n, int32_t a) { return (2 * n + a) / (2 * a); }

struct Edge {
  int32_t found;   // 1: the trace met a background pixel; 0: it left the image
  int32_t ex, ey;  // E = f + b, the doubled midpoint of the last foreground and the first background pixel (-1 when open)
};

// From site (px, py) along s * v, v = p - nearest[p] != 0, s = -1 (near side) or +1 (far side).  bg(x, y): the pixel inside
// the image is background.  Step k moves k pixels along the longer axis of v, so the loop ends after at most max(w, h) steps.
template <typename Bg>
PCP_CW_HD Edge trace(const Bg &bg, int32_t px, int32_t py, int32_t vx, int32_t vy, int32_t s, int32_t w, int32_t h) {
  const int32_t ax = vx < 0 ? -vx : vx, ay = vy < 0 ? -vy : vy, a = ax > ay ? ax : ay;
  const int32_t sx = vx < 0 ? -s : s, sy = vy < 0 ? -s : s;
  const int32_t limit = w > h ? w : h;
  int32_t fx = px, fy = py;
  Edge e{0, -1, -1};
  if (a == 0) return e;
  for (int32_t k = 1; k <= limit; ++k) {
    const int32_t qx = px + sx * rdiv(k * ax, a), qy = py + sy * rdiv(k * ay, a);
    if (qx < 0 || qy < 0 || qx >= w || qy >= h) return e;
    if (bg(qx, qy)) {
      e.found = 1;
      e.ex = fx + qx;
      e.ey = fy + qy;
      return e;
    }
    fx = qx;
    fy = qy;
  }
  return e;
}

// w2d2 = |E_far - E_near|^2 in half-pixel units (each component below 2^15, the sum below 2^31)
PCP_CW_HD uint32_t edge_distance2(const Edge &n, const Edge &f) {
  const int32_t dx = f.ex - n.ex, dy = f.ey - n.ey;
  return static_cast<uint32_t>(dx * dx) + static_cast<uint32_t>(dy * dy);
}

// ---- CW4: members and their quanta ----------------------------------------------------------------------------------------
// (NaN fails every comparison)
PCP_CW_HD bool member_ok(float x, float y, float z) {
  return fabsf(x) < kMaxCoordinate && fabsf(y) < kMaxCoordinate && fabsf(z) < kMaxCoordinate;
}

// rint(c * 2^16), ties to even; the product is exact (a power of two, |c| < 64)
PCP_CW_HD int32_t quantise(float c) {
  const float p = c * kQuantaPerMetre;
#if defined(__HIP_DEVICE_COMPILE__)
  return __float2int_rn(p);
#else
  return static_cast<int32_t>(lrintf(p));  // (the default rounding mode; nothing in the library changes it)
#endif
}

// the ten origin moments of one member, as the words that are summed modulo 2^64
PCP_CW_HD void origin_terms(int32_t qx, int32_t qy, int32_t qz, uint64_t t[kOriginPlanes]) {
  const int64_t x = qx, y = qy, z = qz;
  t[0] = 1;
  t[1] = static_cast<uint64_t>(x);
  t[2] = static_cast<uint64_t>(y);
  t[3] = static_cast<uint64_t>(z);
  t[4] = static_cast<uint64_t>(x * x);
  t[5] = static_cast<uint64_t>(x * y);
  t[6] = static_cast<uint64_t>(x * z);
  t[7] = static_cast<uint64_t>(y * y);
  t[8] = static_cast<uint64_t>(y * z);
  t[9] = static_cast<uint64_t>(z * z);
}

// the window of CW4 along one axis: [max(0, p - R), min(size, p + R))
PCP_CW_HD void window(int32_t p, int32_t radius, int32_t size, int32_t &lo, int32_t &hi) {
  lo = p - radius < 0 ? 0 : p - radius;
  hi = p + radius > size ? size : p + radius;
}

// The sum over rows [y0, y1) and columns [x0, x1) from an inclusive summed-area table taken modulo 2^64; sat(x, y) for
// pixels inside the image.
template <typename Sat>
PCP_CW_HD uint64_t window_sum(const Sat &sat, int32_t x0, int32_t x1, int32_t y0, int32_t y1) {
  if (x1 <= x0 || y1 <= y0) return 0;
  uint64_t s = sat(x1 - 1, y1 - 1);
  if (y0 > 0) s -= sat(x1 - 1, y0 - 1);
  if (x0 > 0) s -= sat(x0 - 1, y1 - 1);
  if (x0 > 0 && y0 > 0) s += sat(x0 - 1, y0 - 1);
  return s;
}

// ---- CW5: recentring ------------------------------------------------------------------------------------------------------
PCP_CW_HD int64_t floor_div(int64_t a, int64_t b /* > 0 */) {
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// o[10]: the window's origin moments modulo 2^64 (n and S1 are the true values: |S1| < 2^39).  m[13] = n r S1' S2'.
PCP_CW_HD void recentre(const uint64_t o[kOriginPlanes], int64_t m[kMomentWords]) {
  const int64_t n = static_cast<int64_t>(o[0]);
  for (int a = 0; a < kMomentWords; ++a) m[a] = 0;
  m[0] = n;
  if (n <= 0) return;
  int64_t r[3];
  uint64_t ru[3];
  for (int a = 0; a < 3; ++a) {
    const int64_t s1 = static_cast<int64_t>(o[1 + a]);
    r[a] = floor_div(2 * s1 + n, 2 * n);
    ru[a] = static_cast<uint64_t>(r[a]);
    m[1 + a] = r[a];
    m[4 + a] = s1 - n * r[a];
  }
  const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
  const uint64_t nu = o[0];
  for (int e = 0; e < 6; ++e) {
    const int a = ia[e], b = ib[e];
    // S2' = S2 - r_a S1_b - r_b S1_a + n r_a r_b, modulo 2^64
    const uint64_t v = ((o[4 + e] - ru[a] * o[1 + b]) - ru[b] * o[1 + a]) + (nu * ru[a]) * ru[b];
    m[7 + e] = static_cast<int64_t>(v);
  }
}

// ---- CW6: covariance and centroid (the eigen solve is pcp_eigen33.hpp's, device only) --------------------------------------
PCP_CW_HD void covariance(const int64_t m[kMomentWords], double C[6]) {
  const double n = static_cast<double>(m[0]);
  const double sx = static_cast<double>(m[4]), sy = static_cast<double>(m[5]), sz = static_cast<double>(m[6]);
  C[0] = static_cast<double>(m[7]) - (sx * sx) / n;
  C[1] = static_cast<double>(m[8]) - (sx * sy) / n;
  C[2] = static_cast<double>(m[9]) - (sx * sz) / n;
  C[3] = static_cast<double>(m[10]) - (sy * sy) / n;
  C[4] = static_cast<double>(m[11]) - (sy * sz) / n;
  C[5] = static_cast<double>(m[12]) - (sz * sz) / n;
}

PCP_CW_HD void centroid(const int64_t m[kMomentWords], double c[3]) {
  const double n = static_cast<double>(m[0]);
  for (int a = 0; a < 3; ++a) c[a] = (static_cast<double>(m[1 + a]) + static_cast<double>(m[4 + a]) / n) * (1.0 / 65536.0);
}

// the normal faces the camera: negated when n . c > 0; returns n . c of the oriented normal
PCP_CW_HD double orient(double n[3], const double c[3]) {
  double nc = (n[0] * c[0] + n[1] * c[1]) + n[2] * c[2];
  if (nc > 0.0) {
    n[0] = -n[0];
    n[1] = -n[1];
    n[2] = -n[2];
    nc = -nc;
  }
  return nc;
}

// ---- CW7: rays ------------------------------------------------------------------------------------------------------------
struct Intrinsics {
  double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// the projection's distortion as the reference writes it (pcp_device.hpp project_uv, written form)
PCP_CW_HD void distort(const Intrinsics &c, double xn, double yn, double &xd, double &yd) {
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

// the projection coordinates of a doubled edge point: the pixel rule truncates, so a pixel's centre is at + 0.5
PCP_CW_HD void edge_uv(int32_t ex, int32_t ey, double &u, double &v) {
  u = static_cast<double>(ex) * 0.5 + 0.5;
  v = static_cast<double>(ey) * 0.5 + 0.5;
}

// The normalised ray (x, y, 1) through (u, v): exactly ten fixed-point steps, then the redistortion test.  A camera whose
// distortion folds back fails the test rather than giving a wrong ray.
PCP_CW_HD bool undistort(const Intrinsics &c, double u, double v, double &x, double &y) {
  const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
  x = x0;
  y = y0;
  for (int it = 0; it < kUndistortSteps; ++it) {
    const double x2 = x * x;
    const double y2 = y * y;
    const double r2 = x2 + y2;
    const double r4 = r2 * r2;
    const double r6 = r2 * r4;
    const double rc = ((1.0 + c.k1 * r2) + c.k2 * r4) + c.k3 * r6;
    const double t1 = (2.0 * x) * y;
    const double t2 = r2 + 2.0 * x2;
    const double t3 = r2 + 2.0 * y2;
    x = (x0 - (c.p1 * t1 + c.p2 * t2)) / rc;
    y = (y0 - (c.p1 * t3 + c.p2 * t1)) / rc;
  }
  double xd, yd;
  distort(c, x, y, xd, yd);
  const double ur = c.fx * xd + c.cx, vr = c.fy * yd + c.cy;
  return fabs(ur - u) <= kReprojectionPx && fabs(vr - v) <= kReprojectionPx;  // (NaN fails)
}

// X = t d on the plane n . (X - c) = 0, d = (x, y, 1); nc = n . c
PCP_CW_HD bool intersect(const double n[3], double nc, double x, double y, double X[3]) {
  const double g = (n[0] * x + n[1] * y) + n[2];
  const double len = sqrt((x * x + y * y) + 1.0);
  if (!(fabs(g) >= kMinIncidence * len)) return false;
  const double t = nc / g;
  if (!(t > 0.0)) return false;
  X[0] = t * x;
  X[1] = t * y;
  X[2] = t;
  return true;
}

// CW7 for one doubled edge point
PCP_CW_HD bool edge_point(const Intrinsics &c, const double n[3], double nc, int32_t ex, int32_t ey, double X[3]) {
  double u, v, x, y;
  edge_uv(ex, ey, u, v);
  if (!undistort(c, u, v, x, y)) return false;
  return intersect(n, nc, x, y, X);
}

// CW8
PCP_CW_HD double width_of(const double a[3], const double b[3]) {
  const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

}  // namespace cw
}  // namespace pcp
