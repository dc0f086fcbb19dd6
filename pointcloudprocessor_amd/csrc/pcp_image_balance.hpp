// pcp_image_balance.hpp -- the per-element arithmetic of the keyframe colour balance ("Image balance", IB1-IB9), one
// copy for the kernels (pcp_image_balance.hip), the CPU form (pcp_image_balance_host) and host/image_balance_selftest.cpp.
//
// What it replaces: the reference's scripts/image_color_balance_autonomous.py and scripts/image_color_balance.py, which run
// cv2.createCLAHE(clipLimit, tileGridSize).apply() on a lightness channel and then cv2.LUT with adjust_gamma's table over a
// keyframe folder before PointCloudProcessor is started.
//
// Stated difference (IB2): the scripts take L of 8-bit Lab as the lightness channel; this stage takes V of the 8-bit HSV
// conversion pcp_hsv.hpp restates (RGB2HSV_b forward, HSV2RGB_native backward), which generateColorMap applies to every keyframe
// anyway.  OpenCV's Lab tables are not restated here, so parity with the scripts' pixels is unpinned, as it is for the HSV
// round trip.  CLAHE follows OpenCV 4.2's imgproc/src/clahe.cpp for CV_8UC1 [upstream: restated from its published source;
// the rules in DESIGN.md are the definition].
//
// fp32 interpolation, every operation rounded on its own: built with -ffp-contract=off like pcp_hsv.hpp.
#pragma once

#include <cmath>
#include <cstdint>

#include "pcp_hsv.hpp"

#if defined(__HIPCC__)
#define PCP_IB_HD __host__ __device__ __forceinline__
#else
#define PCP_IB_HD inline
#endif

namespace pcp {
namespace ib {

constexpr int32_t kMaxTiles = 16;  // IB3: tiles_x, tiles_y in 1..16
constexpr int32_t kBins = 256;
constexpr int32_t kStageClahe = 1, kStageGamma = 2;  // PCP_BALANCE_CLAHE, PCP_BALANCE_GAMMA

// IB3: the tile grid over the (virtually) extended image
struct Grid {
  int32_t w, h, tiles_x, tiles_y;
  int32_t tw, th, total;  // tile size in extended pixels
  float inv_tw, inv_th;   // IB7: f32(1.0f / tw), f32(1.0f / th)
  float lut_scale;        // IB6: f32(255.0f / (float)total)
};

// 0: fine; 1: tiles outside 1..16 or an empty image; 2: a reflected index would leave the image
PCP_IB_HD int make_grid(int32_t w, int32_t h, int32_t tiles_x, int32_t tiles_y, Grid *g) {
  if (w < 1 || h < 1 || tiles_x < 1 || tiles_x > kMaxTiles || tiles_y < 1 || tiles_y > kMaxTiles) return 1;
  int32_t ext_x = 0, ext_y = 0;
  if (w % tiles_x != 0 || h % tiles_y != 0) {  // as clahe.cpp: a side that divides evenly is then extended by a whole tile count
    ext_x = tiles_x - w % tiles_x;
    ext_y = tiles_y - h % tiles_y;
  }
  if (ext_x >= w || ext_y >= h) return 2;
  g->w = w;
  g->h = h;
  g->tiles_x = tiles_x;
  g->tiles_y = tiles_y;
  g->tw = (w + ext_x) / tiles_x;
  g->th = (h + ext_y) / tiles_y;
  g->total = g->tw * g->th;
  g->inv_tw = 1.0f / static_cast<float>(g->tw);
  g->inv_th = 1.0f / static_cast<float>(g->th);
  g->lut_scale = 255.0f / static_cast<float>(g->total);
  return 0;
}

// IB3: BORDER_REFLECT_101 past the far edge (i < 2 n - 1 by make_grid)
PCP_IB_HD int32_t reflect101(int32_t i, int32_t n) { return i < n ? i : 2 * (n - 1) - i; }

// IB5: the clip count of a tile; 0 = no clipping
PCP_IB_HD int32_t clip_count(float clip_limit, int32_t total) {
  if (!(clip_limit > 0.0f)) return 0;
  const double c = static_cast<double>(clip_limit) * total / 256;
  const int32_t clip = c >= 2147483647.0 ? 2147483647 : static_cast<int32_t>(c);
  return clip > 1 ? clip : 1;
}

// IB5: what a bin holds above the clip count (summed over the tile's bins: `clipped`)
PCP_IB_HD int32_t excess(int32_t count, int32_t clip) { return clip > 0 && count > clip ? count - clip : 0; }

// IB5: bin i after clipping and redistribution, in closed form: the serial walk `for (i = 0; i < 256 && residual > 0;
// i += step, --residual) ++hist[i]` reaches bin i iff i % step == 0 and i / step < residual (residual < 256, so
// step * residual <= 256 and the walk never stops at the 256 bound first)
PCP_IB_HD int32_t redistributed(int32_t count, int32_t i, int32_t clip, int32_t clipped) {
  if (clip <= 0) return count;
  int32_t v = count > clip ? clip : count;
  const int32_t batch = clipped / kBins;
  const int32_t residual = clipped - batch * kBins;
  v += batch;
  if (residual != 0) {
    const int32_t q = kBins / residual;
    const int32_t step = q > 1 ? q : 1;
    if (i % step == 0 && i / step < residual) ++v;
  }
  return v;
}

// IB6: one LUT byte from the inclusive prefix sum
PCP_IB_HD uint32_t lut_entry(int32_t cum, float lut_scale) { return sat_u8_from_float(static_cast<float>(cum) * lut_scale); }

// IB7: the two tiles and the weights of one coordinate
struct Weights {
  int32_t t1, t2;
  float a, a1;
};
PCP_IB_HD Weights weights(int32_t x, float inv_t, int32_t tiles) {
  const float tf = static_cast<float>(x) * inv_t - 0.5f;
  const float fl = floorf(tf);
  int32_t t1 = static_cast<int32_t>(fl);
  int32_t t2 = t1 + 1;
  Weights r;
  r.a = tf - fl;
  r.a1 = 1.0f - r.a;
  r.t1 = t1 > 0 ? t1 : 0;
  r.t2 = t2 < tiles - 1 ? t2 : tiles - 1;
  return r;
}

// IB7: V' from the four LUT bytes
PCP_IB_HD uint32_t interpolate(uint32_t l11, uint32_t l12, uint32_t l21, uint32_t l22, const Weights &wx, const Weights &wy) {
  const float top = static_cast<float>(l11) * wx.a1 + static_cast<float>(l12) * wx.a;
  const float bottom = static_cast<float>(l21) * wx.a1 + static_cast<float>(l22) * wx.a;
  return sat_u8_from_float(top * wy.a1 + bottom * wy.a);
}

// IB8: adjust_gamma's table, fp64, truncated (host only: built once per setting, 256 bytes)
inline void gamma_table(float gamma, uint8_t out[256]) {
  const double inv = 1.0 / static_cast<double>(gamma);
  for (int i = 0; i < 256; ++i) {
    const double v = std::pow(i / 255.0, inv) * 255.0;
    out[i] = static_cast<uint8_t>(v >= 255.0 ? 255 : (v <= 0.0 ? 0 : static_cast<int>(v)));
  }
}

// IB1: one pixel through steps 1-4 given the four LUTs of its neighbourhood (lut: [tiles_y][tiles_x][256]); gamma may be null
PCP_IB_HD uint32_t lookup4(const uint8_t *lut, int32_t tiles_x, const Weights &wx, const Weights &wy, uint32_t V) {
  const uint8_t *r1 = lut + static_cast<int64_t>(wy.t1) * tiles_x * kBins, *r2 = lut + static_cast<int64_t>(wy.t2) * tiles_x * kBins;
  return interpolate(r1[wx.t1 * kBins + V], r1[wx.t2 * kBins + V], r2[wx.t1 * kBins + V], r2[wx.t2 * kBins + V], wx, wy);
}

}  // namespace ib
}  // namespace pcp
