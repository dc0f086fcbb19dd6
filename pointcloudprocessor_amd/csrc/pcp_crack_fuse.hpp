// pcp_crack_fuse.hpp -- the per-element arithmetic of the crack widths on the map ("Crack widths on the map",
// CF1-CF6 and CC1-CC6), one copy for the kernels (pcp_crack_fuse.hip), the CPU forms (pcp_crack_fuse_host,
// pcp_crack_components_host) and the host self-test (host/crack_fuse_selftest.cpp): the width quantum, the update of one
// point's state by one keyframe, the fused results, the link test and the ordered-integer form of a coordinate.  Every
// result is an exact integer or a correctly rounded conversion of one, so nothing depends on the order of the keyframes,
// of the points or of a traversal.  Build without floating-point contraction.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define PCP_CF_HD __host__ __device__ __forceinline__
#else
#define PCP_CF_HD inline
#endif

#include "pcp_normals.hpp"

namespace pcp {
namespace cf {

constexpr uint8_t kCentreFlag = 2, kWidthFlag = 64;   // CW9's CENTRE and WIDTH bits of the flag byte
constexpr float kQuantaPerMetre = 1048576.0f;         // CF3: 2^20, the quantum is ~0.95 um
constexpr float kClampWidth = 2048.0f;                // CF3: widths from here on take the largest quantum
constexpr uint32_t kClampQ = 0x7fffffffu;             // 2^31 - 1
constexpr uint32_t kNoMin = 0xffffffffu;              // min_q of a point without a credited keyframe
constexpr uint64_t kNoKey = ~uint64_t(0);             // best_key likewise
constexpr int32_t kMinViewsLo = 1, kMinViewsHi = 4096;  // CC1
constexpr int64_t kHostMaxPoints = 65536;             // pcp_crack_components_host

// ---- CF3: the quantum of a width (metres, >= 0) ----------------------------------------------------------------------------
// (a NaN takes the clamp: it fails the comparison)
PCP_CF_HD uint32_t quantum(float width) {
  if (!(width < kClampWidth)) return kClampQ;
  const float p = width * kQuantaPerMetre;  // exact: a power of two, p < 2^31
#if defined(__HIP_DEVICE_COMPILE__)
  return __float2uint_rn(p);
#else
  return static_cast<uint32_t>(lrintf(p));  // (the default rounding mode; nothing in the library changes it)
#endif
}

// ---- the state of one map point -------------------------------------------------------------------------------------------
struct State {
  uint32_t seen, views, centres, min_q, max_q, best_q;
  uint64_t sum_q, best_key;
};

PCP_CF_HD void clear(State &s) {
  s.seen = s.views = s.centres = 0;
  s.min_q = kNoMin;
  s.max_q = 0;
  s.best_q = 0;
  s.sum_q = 0;
  s.best_key = kNoKey;
}

PCP_CF_HD uint64_t key_of(uint32_t range_bits, int32_t frame) {
  return (static_cast<uint64_t>(range_bits) << 32) | static_cast<uint32_t>(frame);
}

// CF2 / CF4: keyframe `frame` sees the point at a pixel with flag byte `flag` and width `width`, at fp32 range `range_bits`
// (positive: the bits order as the values).  true iff the keyframe is credited.
PCP_CF_HD bool update(State &s, uint8_t flag, float width, uint32_t range_bits, int32_t frame) {
  s.seen += 1;
  if (!(flag & kWidthFlag)) return false;
  const uint32_t q = quantum(width);
  s.views += 1;
  if (flag & kCentreFlag) s.centres += 1;
  s.sum_q += q;
  if (q < s.min_q) s.min_q = q;
  if (q > s.max_q) s.max_q = q;
  const uint64_t key = key_of(range_bits, frame);
  if (key < s.best_key) {
    s.best_key = key;
    s.best_q = q;
  }
  return true;
}

// ---- CF5 ------------------------------------------------------------------------------------------------------------------
// the mean quantum rounded to nearest, halves up: floor((2 sum + views) / (2 views)); sum < 2^62
PCP_CF_HD uint32_t fused_w(uint64_t sum_q, uint32_t views) {
  if (views == 0) return 0;
  return static_cast<uint32_t>((2 * sum_q + views) / (2 * static_cast<uint64_t>(views)));
}

PCP_CF_HD float width_mean(uint64_t sum_q, uint32_t views) {
  if (views == 0) return 0.0f;
  return static_cast<float>((static_cast<double>(sum_q) / static_cast<double>(views)) * (1.0 / 1048576.0));
}

PCP_CF_HD float width_best(uint32_t best_q, uint32_t views) {
  return views == 0 ? 0.0f : static_cast<float>(static_cast<double>(best_q) * (1.0 / 1048576.0));
}

PCP_CF_HD int32_t best_frame(uint64_t best_key, uint32_t views) {
  return views == 0 ? -1 : static_cast<int32_t>(static_cast<uint32_t>(best_key & 0xffffffffu));
}

// ---- CC1 / CC2 ------------------------------------------------------------------------------------------------------------
PCP_CF_HD bool min_views_ok(int32_t v) { return v >= kMinViewsLo && v <= kMinViewsHi; }

PCP_CF_HD bool crack_point(uint32_t views, int32_t min_views, float x, float y, float z) {
  return views >= static_cast<uint32_t>(min_views) && gn::finite3(x, y, z);
}

// GN's neighbour rule on d = fl32(p_j - p_i): symmetric, because fl32(a - b) = -fl32(b - a)
PCP_CF_HD bool linked(float dx, float dy, float dz, float t) {
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  return d2 <= t;
}

// ---- CC4: float min / max as unsigned integers ----------------------------------------------------------------------------
// order_bits is increasing in the value of a finite float (and puts -0 below +0); value_of inverts it
PCP_CF_HD uint32_t order_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t b = __float_as_uint(f);
#else
  uint32_t b;
  std::memcpy(&b, &f, 4);
#endif
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

PCP_CF_HD float value_of(uint32_t o) {
  const uint32_t b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float f;
  std::memcpy(&f, &b, 4);
  return f;
#endif
}

struct Box {
  uint32_t lo[3], hi[3];  // order_bits of the smallest / largest coordinate per axis
};

PCP_CF_HD void clear(Box &b) {
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = 0xffffffffu;
    b.hi[a] = 0;
  }
}

PCP_CF_HD void add(Box &b, float x, float y, float z) {
  const uint32_t o[3] = {order_bits(x), order_bits(y), order_bits(z)};
  for (int a = 0; a < 3; ++a) {
    if (o[a] < b.lo[a]) b.lo[a] = o[a];
    if (o[a] > b.hi[a]) b.hi[a] = o[a];
  }
}

// ---- CC1-CC3 by brute force over the pairs (the core of pcp_crack_components_host) -----------------------------------------
// label[i] = lowest input index of i's component, -1 for a point that is no crack point; returns the number of components.
// A plain union-find whose roots are the lowest indices: the smaller root always becomes the parent.  Host only.
inline int64_t label_brute(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float t, int32_t *label) {
  std::vector<int32_t> parent(static_cast<size_t>(n));
  std::vector<int32_t> list;
  for (int64_t i = 0; i < n; ++i) {
    parent[static_cast<size_t>(i)] = static_cast<int32_t>(i);
    if (crack_point(views[i], min_views, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) list.push_back(static_cast<int32_t>(i));
  }
  auto find = [&](int32_t v) {
    while (parent[static_cast<size_t>(v)] != v) {
      parent[static_cast<size_t>(v)] = parent[static_cast<size_t>(parent[static_cast<size_t>(v)])];
      v = parent[static_cast<size_t>(v)];
    }
    return v;
  };
  for (size_t a = 0; a < list.size(); ++a) {
    const int32_t i = list[a];
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    for (size_t b = a + 1; b < list.size(); ++b) {
      const int32_t j = list[b];
      if (!linked(xyz[3 * j] - x, xyz[3 * j + 1] - y, xyz[3 * j + 2] - z, t)) continue;
      const int32_t ri = find(i), rj = find(j);
      if (ri < rj) parent[static_cast<size_t>(rj)] = ri;
      if (rj < ri) parent[static_cast<size_t>(ri)] = rj;
    }
  }
  for (int64_t i = 0; i < n; ++i) label[i] = -1;
  int64_t components = 0;
  for (int32_t i : list) {
    label[i] = find(i);
    if (label[i] == i) ++components;
  }
  return components;
}

}  // namespace cf
}  // namespace pcp
