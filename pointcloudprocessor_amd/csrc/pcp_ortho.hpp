// pcp_ortho.hpp -- the per-element arithmetic of the orthographic maps ("Orthographic maps", OM1-OM8), one copy
// for the kernels (pcp_ortho.hip), the CPU form (pcp_ortho_host) and host/ortho_selftest.cpp.  fp32 throughout, built with
// -ffp-contract=off: every product and every sum below is rounded on its own.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCP_OM_HD __host__ __device__ __forceinline__
#else
#define PCP_OM_HD inline
#endif

namespace pcp {
namespace om {

constexpr int32_t kMaxSide = 16384;                  // OM1: the limits of the mask distance maps, whose row stage fills the map
constexpr int64_t kMaxPixels = int64_t(1) << 26;
constexpr int32_t kMaxFill = 1024;                   // OM6
constexpr unsigned long long kEmptyKey = ~0ull;      // OM3
constexpr uint32_t kNoIndex = 0xffffffffu;           // OM7
constexpr int64_t kMaxIndexEnd = 0xffffffffll;       // OM3: index_base + n <= 2^32 - 1, so no key is the empty one

// OM1: the frame as the kernels take it (the caller's values and inv = f32(1.0f / gsd))
struct Frame {
  float o[3], u[3], v[3], n[3];
  float inv, wf, hf, d_min, d_max;
  int32_t w, h;
};

PCP_OM_HD float inverse_gsd(float gsd) { return 1.0f / gsd; }

PCP_OM_HD uint32_t float_bits(float f) {
  uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
  b = __float_as_uint(f);
#else
  std::memcpy(&b, &f, 4);
#endif
  return b;
}
PCP_OM_HD float bits_float(uint32_t b) {
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  f = __uint_as_float(b);
#else
  std::memcpy(&f, &b, 4);
#endif
  return f;
}

// OM3: the order-preserving image of a float's bits (no NaN comes here): a < b as floats  <=>  ord(a) < ord(b), with -0 below +0
PCP_OM_HD uint32_t ord(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
PCP_OM_HD uint32_t unord(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }

// OM2: the dot product of d with a column c in GM4's association
PCP_OM_HD float dot3(const float d[3], const float c[3]) { return d[0] * c[0] + (d[1] * c[1] + d[2] * c[2]); }

PCP_OM_HD bool finite_bits(float f) { return (float_bits(f) & 0x7f800000u) != 0x7f800000u; }

// OM2: pixel and depth bits of a point; false: not a contributor (the has bit is the caller's to check).  The comparisons
// against the raster are made in float before any conversion; a depth of -0 leaves as +0.
PCP_OM_HD bool project(const Frame &f, float x, float y, float z, int32_t *pixel, uint32_t *depth_bits) {
  if (!(finite_bits(x) && finite_bits(y) && finite_bits(z))) return false;
  const float d[3] = {x - f.o[0], y - f.o[1], z - f.o[2]};
  const float s = dot3(d, f.u), t = dot3(d, f.v), depth = dot3(d, f.n);
  const float a = s * f.inv, b = t * f.inv;
  if (!(a >= 0.0f && a < f.wf && b >= 0.0f && b < f.hf)) return false;
  if (!(depth >= f.d_min && depth <= f.d_max)) return false;
  const int32_t col = static_cast<int32_t>(floorf(a)), row = static_cast<int32_t>(floorf(b));
  *pixel = row * f.w + col;
  const uint32_t db = float_bits(depth);
  *depth_bits = (db & 0x7fffffffu) ? db : 0u;
  return true;
}

// OM3: the key of a contributor and what it gives back
PCP_OM_HD unsigned long long key_of(uint32_t depth_bits, uint32_t g) {
  return (static_cast<unsigned long long>(ord(depth_bits)) << 32) | g;
}
PCP_OM_HD uint32_t key_index(unsigned long long key) { return static_cast<uint32_t>(key); }
PCP_OM_HD float key_depth(unsigned long long key) { return bits_float(unord(static_cast<uint32_t>(key >> 32))); }

// OM4: the payload word of a contributor
PCP_OM_HD uint32_t payload_of(uint32_t packed_word, uint32_t label) { return (packed_word & 0x00ffffffu) | (label << 24); }

// OM6: the pixel an empty pixel is filled from, given the distance transform's result for it (occupied pixels as background)
PCP_OM_HD int32_t fill_source(uint32_t d2, int32_t nearest, int32_t radius) {
  return (nearest >= 0 && d2 <= static_cast<uint32_t>(radius * radius)) ? nearest : -1;
}

// OM1, host only: the smallest gsd (to a part in 10^4) at which an extent of ew x eh metres plus `extra` pixels a side fits
inline double fit_gsd(double ew, double eh, double extra) {
  double g = std::fmax(std::fmax(ew, eh) / kMaxSide, std::sqrt(ew * eh / static_cast<double>(kMaxPixels)));
  if (!(g > 0.0)) return 0.0;
  for (int k = 0; k < 100000; ++k, g *= 1.0001) {
    const double w = std::ceil(ew / g) + extra, h = std::ceil(eh / g) + extra;
    if (w <= kMaxSide && h <= kMaxSide && w * h <= static_cast<double>(kMaxPixels)) break;
  }
  return g;
}

// OM1, host only.  0: fine; 1: a non-finite value, a gsd outside [1e-4, 1], an empty raster or window, axes that are not
// orthonormal and right-handed within 1e-3 (*why says which); 2: a raster past the limits, *fit_gsd = the gsd at which the
// same extent fits.
inline int frame_check(const float o[3], const float u[3], const float v[3], const float n[3], float gsd, int64_t w, int64_t h,
                       float d_min, float d_max, const char **why, double *fit_gsd) {
  *fit_gsd = 0.0;
  auto refuse = [&](const char *what, int code) {
    *why = what;
    return code;
  };
  bool finite = std::isfinite(gsd) && std::isfinite(d_min) && std::isfinite(d_max);
  for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(o[a]) && std::isfinite(u[a]) && std::isfinite(v[a]) && std::isfinite(n[a]);
  if (!finite) return refuse("a value of the frame is not finite", 1);
  if (!(gsd >= 1e-4f && gsd <= 1.0f)) return refuse("gsd outside [1e-4, 1]", 1);
  if (!(d_min < d_max)) return refuse("the depth window is empty (d_min < d_max is required)", 1);
  if (w < 1 || h < 1) return refuse("width and height start at 1", 1);
  const double U[3] = {u[0], u[1], u[2]}, V[3] = {v[0], v[1], v[2]}, N[3] = {n[0], n[1], n[2]};
  auto dot = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  const double cross[3] = {U[1] * V[2] - U[2] * V[1], U[2] * V[0] - U[0] * V[2], U[0] * V[1] - U[1] * V[0]};
  const double tol = 1e-3;
  bool ok = std::fabs(dot(U, U) - 1.0) <= tol && std::fabs(dot(V, V) - 1.0) <= tol && std::fabs(dot(N, N) - 1.0) <= tol &&
            std::fabs(dot(U, V)) <= tol && std::fabs(dot(U, N)) <= tol && std::fabs(dot(V, N)) <= tol;
  for (int a = 0; a < 3; ++a) ok = ok && std::fabs(cross[a] - N[a]) <= tol;
  if (!ok) return refuse("the axes are not orthonormal and right-handed (u x v = n) within 1e-3", 1);
  if (w > kMaxSide || h > kMaxSide || w * h > kMaxPixels) {
    *fit_gsd = om::fit_gsd(static_cast<double>(w) * gsd, static_cast<double>(h) * gsd, 0.0);
    return refuse("the raster exceeds 16384 a side or 2^26 pixels", 2);
  }
  return 0;
}

}  // namespace om
}  // namespace pcp
