// pcp_ortho_texture.hpp -- the surface point behind a fine pixel of an orthophoto ("Orthophotos", OT2-OT3), one copy
// for the kernel (pcp_ortho_texture.hip), the host form (pcp_ortho_texture_points_host) and host/ortho_texture_selftest.cpp.
// fp32 throughout, built with -ffp-contract=off: every product, quotient and sum below is rounded on its own.
#pragma once

#include <cmath>
#include <cstdint>

#include "pcp_ortho.hpp"

namespace pcp {
namespace ot {

constexpr int32_t kMaxScale = 16;                    // OT2
constexpr int32_t kMaxViews = 5;                     // OT2: the length of the reference's list
constexpr int64_t kMaxFine = int64_t(1) << 28;       // OT2: fine pixels of one call
constexpr int32_t kMaxFrames = 32766;                // OT2: the view layer is int16

// OT2: the call's raster -- the rectangle in ortho pixels (already resolved: never "the whole raster") and the fine pitch
struct Raster {
  int32_t k, x0, y0, w, h;
  int32_t interpolate;
  float max_step;
};

// OT2.  0: fine; 1: PCP_ERR_INVALID (*why says what); 2: PCP_ERR_RANGE, *fit = the largest scale at which the rectangle fits.
// W x H: the ortho raster.  On 0 *out is the resolved raster.
inline int raster_check(int32_t W, int32_t H, int32_t scale, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t views, int32_t interpolate,
                        float max_step, Raster *out, const char **why, int32_t *fit) {
  *fit = 0;
  auto refuse = [&](const char *what) {
    *why = what;
    return 1;
  };
  if (scale < 1 || scale > kMaxScale) return refuse("scale outside 1..16");
  if (views < 1 || views > kMaxViews) return refuse("views outside 1..5");
  if (!(std::isfinite(max_step) && max_step > 0.0f)) return refuse("max_step is not a finite number above 0");
  if (w == 0 && h == 0) {
    if (x0 != 0 || y0 != 0) return refuse("the whole raster (w == 0 and h == 0) starts at x0 == 0, y0 == 0");
    w = W;
    h = H;
  }
  if (w < 1 || h < 1) return refuse("one of w, h is zero or negative");
  if (x0 < 0 || y0 < 0 || x0 > W - w || y0 > H - h) return refuse("the rectangle leaves the ortho raster");
  const int64_t px = static_cast<int64_t>(w) * h;
  if (px * scale * scale > kMaxFine) {
    int32_t k = scale;
    while (k > 1 && px * k * k > kMaxFine) --k;
    *fit = k;  // (w * h <= 2^26: scale 1 and 2 always fit)
    *why = "more than 2^28 fine pixels";
    return 2;
  }
  *out = Raster{scale, x0, y0, w, h, interpolate ? 1 : 0, max_step};
  return 0;
}

PCP_OM_HD int32_t sign_of(int32_t a) { return (a > 0) - (a < 0); }

// OT3: the depth behind fine pixel (Xg, Yg) of the whole fine raster (Xg = x0 * k + X).  source: the finished map's source
// image, W x H; depth_at(p): the depth the map holds at SOURCE pixel p (an occupied one).  false: no surface.
template <typename DepthAt>
PCP_OM_HD bool surface_depth(const Raster &r, int32_t W, int32_t H, const int32_t *source, DepthAt depth_at, int32_t Xg, int32_t Yg, float *out) {
  const int32_t k = r.k;
  const int32_t c = Xg / k, row = Yg / k;
  const int32_t s00 = source[static_cast<int64_t>(row) * W + c];
  if (s00 < 0) return false;
  const float d00 = depth_at(s00);
  *out = d00;
  if (!r.interpolate) return true;
  const int32_t a = 2 * (Xg - c * k) + 1 - k, b = 2 * (Yg - row * k) + 1 - k;
  if (a == 0 && b == 0) return true;  // (the centre of an odd k: every neighbour is the parent)
  const int32_t c2 = c + sign_of(a), r2 = row + sign_of(b);
  if (c2 < 0 || c2 >= W || r2 < 0 || r2 >= H) return true;
  auto near = [&](float d) { return fabsf(d - d00) <= r.max_step; };
  float d10 = d00, d01 = d00, d11 = d00;
  if (a != 0) {
    const int32_t s = source[static_cast<int64_t>(row) * W + c2];
    if (s < 0) return true;
    d10 = depth_at(s);
    if (!near(d10)) return true;
  }
  if (b != 0) {
    const int32_t s = source[static_cast<int64_t>(r2) * W + c];
    if (s < 0) return true;
    d01 = depth_at(s);
    if (!near(d01)) return true;
  }
  if (a != 0 && b != 0) {
    const int32_t s = source[static_cast<int64_t>(r2) * W + c2];
    if (s < 0) return true;
    d11 = depth_at(s);
    if (!near(d11)) return true;
  } else if (a == 0) {
    d11 = d01;  // (d10 == d00 already)
  } else {
    d11 = d10;  // b == 0 (d01 == d00 already)
  }
  const float two_k = static_cast<float>(2 * k);
  const float wx = static_cast<float>(a < 0 ? -a : a) / two_k, wy = static_cast<float>(b < 0 ? -b : b) / two_k;
  const float top = d00 + wx * (d10 - d00);
  const float bot = d01 + wx * (d11 - d01);
  *out = top + wy * (bot - top);
  return true;
}

// OT3: the position of the surface point of fine pixel (Xg, Yg) at depth d; f: the ortho frame as the caller gave it
PCP_OM_HD void surface_point(const float o[3], const float u[3], const float v[3], const float n[3], float gsd, int32_t k, int32_t Xg,
                             int32_t Yg, float d, float p[3]) {
  const float gk = gsd / static_cast<float>(k);
  const float s = (static_cast<float>(Xg) + 0.5f) * gk, t = (static_cast<float>(Yg) + 0.5f) * gk;
  for (int a = 0; a < 3; ++a) p[a] = o[a] + ((s * u[a] + t * v[a]) + d * n[a]);
}

}  // namespace ot
}  // namespace pcp
