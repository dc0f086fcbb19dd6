// pcp_crack_skeleton.hpp -- the arithmetic of the crack skeletons on the map ("Crack skeletons on the map",
// CS1-CS9), one copy for the kernels (pcp_crack_skeleton.hip), the CPU form (pcp_crack_skeleton_host) and the host self-test
// (host/crack_skeleton_selftest.cpp): the band of an arc position, the limits of the step, the quantum of a coordinate, the
// key of an edge, and the whole stage by brute force over the pairs with a sequential union-find and a std::map of edges.
// Every result is an integer that has one value whatever computes it.  Build without floating-point contraction.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "pcp_crack_length.hpp"

namespace pcp {
namespace cs {

constexpr int kNodeWords = 10;  // CS4: crack_row band points sum_w min_w max_w sum_qx sum_qy sum_qz degree
constexpr int kEdgeWords = 3;   // CS5: u v links
constexpr int kCrackWords = 6;  // CS6: nodes edges ends junctions loops max_degree
constexpr float kMaxStep = 16.0f;         // CS2
constexpr float kMaxCoord = 1048576.0f;   // CS4: 2^20 m
constexpr uint64_t kNoKey = ~uint64_t(0);  // an empty slot of the edge set (no key has u = 2^32 - 1)

// ---- CS2 ------------------------------------------------------------------------------------------------------------------
// the step in units of 2^-20 m, truncated (0 < step <= 16: the product is exact in fp64 and below 2^24)
PCP_CF_HD uint64_t step_q_of(float step) { return static_cast<uint64_t>(static_cast<double>(step) * 1048576.0); }

// the largest weight CL2 gives a link under threshold t (cl::weight is monotone in d2, and d2 <= t)
PCP_CF_HD uint64_t w_max_of(float t) { return cl::isqrt(static_cast<uint64_t>(static_cast<double>(t) * 1099511627776.0)); }

PCP_CF_HD bool step_q_ok(uint64_t step_q, float t) { return step_q >= 1 && step_q >= w_max_of(t); }

// (a NaN fails the first comparison)
PCP_CF_HD bool step_ok(float step, float t) { return step > 0.0f && step <= kMaxStep && step_q_ok(step_q_of(step), t); }

PCP_CF_HD uint64_t band(uint64_t pos, uint64_t step_q) { return pos / step_q; }

// ---- CS4: the quantum of a coordinate, floor(x * 2^20); |x| <= 2^20 m gives |q| <= 2^40 --------------------------------------
PCP_CF_HD bool coord_ok(float x) { return fabsf(x) <= kMaxCoord; }
PCP_CF_HD int64_t quant(float x) { return static_cast<int64_t>(floor(static_cast<double>(x) * 1048576.0)); }

// sums of `points` quanta of coordinates up to `largest` (metres, >= 0) stay below 2^62
inline bool sums_fit(int64_t points, float largest) {
  return static_cast<double>(points) * (static_cast<double>(largest) * 1048576.0 + 1.0) < 4611686018427387904.0;
}

// ---- CS5: u = the row of the node in the lower band, v = the row of the other; the keys order as (u, v) does -------------------
PCP_CF_HD uint64_t edge_key(int32_t u, int32_t v) { return (static_cast<uint64_t>(static_cast<uint32_t>(u)) << 32) | static_cast<uint32_t>(v); }
PCP_CF_HD int32_t key_u(uint64_t key) { return static_cast<int32_t>(key >> 32); }
PCP_CF_HD int32_t key_v(uint64_t key) { return static_cast<int32_t>(key & 0xffffffffu); }

// ---- CS7: host arithmetic on the integers ---------------------------------------------------------------------------------
inline double centroid(int64_t sum_q, int64_t points) { return (static_cast<double>(sum_q) / static_cast<double>(points)) * (1.0 / 1048576.0); }

// ---- the whole stage on the host (the core of pcp_crack_skeleton_host) ----------------------------------------------------
struct HostResult {
  std::vector<int32_t> node;    // n
  std::vector<int32_t> ids;     // N
  std::vector<int64_t> nodes;   // 10 N
  std::vector<int64_t> edges;   // 3 E
  std::vector<int64_t> cracks;  // 6 C
};

enum Brute { kBruteOk = 0, kBruteRange = 1, kBruteLoops = 2 };

// xyz: n x 3; views, sum_q (nullable: every fused width 0): n.  Host only; quadratic in the crack points.  lengths (nullable):
// takes the length stage's result the skeleton was made from (the branch stage reads its ends and pos).
inline Brute skeleton_brute(int64_t n, const float *xyz, const uint32_t *views, const uint64_t *sum_q, int32_t min_views, float t,
                            uint64_t step_q, HostResult &out, cl::HostResult *lengths = nullptr) {
  const size_t sn = static_cast<size_t>(n);
  cl::HostResult own;
  cl::HostResult &len = lengths ? *lengths : own;
  cl::lengths_brute(n, xyz, views, sum_q, min_views, t, len);  // CS1: pos, and the ids of the cracks in table order
  std::vector<int32_t> list;
  for (int64_t i = 0; i < n; ++i)
    if (len.pos[static_cast<size_t>(i)] != cl::kNoPos) list.push_back(static_cast<int32_t>(i));
  float largest = 0.0f;
  for (int32_t i : list)
    for (int a = 0; a < 3; ++a) {
      if (!coord_ok(xyz[3 * static_cast<size_t>(i) + a])) return kBruteRange;
      largest = std::max(largest, fabsf(xyz[3 * static_cast<size_t>(i) + a]));
    }
  if (!sums_fit(static_cast<int64_t>(list.size()), largest)) return kBruteRange;
  std::vector<uint64_t> bnd(sn, 0);
  for (int32_t i : list) bnd[static_cast<size_t>(i)] = band(len.pos[static_cast<size_t>(i)], step_q);
  // two union-finds whose roots are the lowest indices: all links (the crack), the links inside a band (the node)
  std::vector<int32_t> whole(sn), inner(sn);
  for (size_t i = 0; i < sn; ++i) whole[i] = inner[i] = static_cast<int32_t>(i);
  auto find = [](std::vector<int32_t> &parent, int32_t v) {
    while (parent[static_cast<size_t>(v)] != v) {
      parent[static_cast<size_t>(v)] = parent[static_cast<size_t>(parent[static_cast<size_t>(v)])];
      v = parent[static_cast<size_t>(v)];
    }
    return v;
  };
  auto unite = [&](std::vector<int32_t> &parent, int32_t i, int32_t j) {
    const int32_t ri = find(parent, i), rj = find(parent, j);
    if (ri < rj) parent[static_cast<size_t>(rj)] = ri;
    if (rj < ri) parent[static_cast<size_t>(ri)] = rj;
  };
  auto linked = [&](int32_t i, int32_t j) {
    const float *p = xyz + 3 * static_cast<size_t>(i), *q = xyz + 3 * static_cast<size_t>(j);
    return cf::linked(q[0] - p[0], q[1] - p[1], q[2] - p[2], t);
  };
  for (size_t a = 0; a < list.size(); ++a)
    for (size_t b = a + 1; b < list.size(); ++b) {
      const int32_t i = list[a], j = list[b];
      if (!linked(i, j)) continue;
      unite(whole, i, j);
      if (bnd[static_cast<size_t>(i)] == bnd[static_cast<size_t>(j)]) unite(inner, i, j);  // CS3
    }
  out.node.assign(sn, -1);
  out.ids.clear();
  std::vector<int32_t> node_row(sn, -1), crack_row(sn, -1);
  for (size_t r = 0; r < len.ids.size(); ++r) crack_row[static_cast<size_t>(len.ids[r])] = static_cast<int32_t>(r);
  for (int32_t i : list) {
    const int32_t root = find(inner, i);
    out.node[static_cast<size_t>(i)] = root;
    if (root == i) {
      node_row[static_cast<size_t>(i)] = static_cast<int32_t>(out.ids.size());
      out.ids.push_back(i);
    }
  }
  const size_t rows = out.ids.size(), cracks = len.ids.size();
  out.nodes.assign(static_cast<size_t>(kNodeWords) * rows, 0);
  for (size_t r = 0; r < rows; ++r) out.nodes[kNodeWords * r + 4] = INT64_MAX;
  for (int32_t i : list) {  // CS4
    const size_t si = static_cast<size_t>(i);
    int64_t *row = out.nodes.data() + static_cast<size_t>(kNodeWords) * static_cast<size_t>(node_row[static_cast<size_t>(out.node[si])]);
    const int64_t w = sum_q ? static_cast<int64_t>(cf::fused_w(sum_q[si], views[si])) : 0;
    row[0] = crack_row[static_cast<size_t>(find(whole, i))];
    row[1] = static_cast<int64_t>(bnd[si]);
    row[2] += 1;
    row[3] += w;
    row[4] = std::min(row[4], w);
    row[5] = std::max(row[5], w);
    for (int a = 0; a < 3; ++a) row[6 + a] += quant(xyz[3 * si + a]);
  }
  std::map<uint64_t, int64_t> edges;  // CS5
  for (size_t a = 0; a < list.size(); ++a)
    for (size_t b = a + 1; b < list.size(); ++b) {
      const int32_t i = list[a], j = list[b];
      const int32_t ni = node_row[static_cast<size_t>(out.node[static_cast<size_t>(i)])];
      const int32_t nj = node_row[static_cast<size_t>(out.node[static_cast<size_t>(j)])];
      if (ni == nj || !linked(i, j)) continue;
      const bool i_low = bnd[static_cast<size_t>(i)] < bnd[static_cast<size_t>(j)];
      edges[i_low ? edge_key(ni, nj) : edge_key(nj, ni)] += 1;
    }
  out.edges.clear();
  out.cracks.assign(static_cast<size_t>(kCrackWords) * cracks, 0);
  for (const auto &e : edges) {
    const int32_t u = key_u(e.first), v = key_v(e.first);
    out.edges.push_back(u);
    out.edges.push_back(v);
    out.edges.push_back(e.second);
    out.nodes[kNodeWords * static_cast<size_t>(u) + 9] += 1;
    out.nodes[kNodeWords * static_cast<size_t>(v) + 9] += 1;
    out.cracks[kCrackWords * static_cast<size_t>(out.nodes[kNodeWords * static_cast<size_t>(u)]) + 1] += 1;
  }
  for (size_t r = 0; r < rows; ++r) {  // CS6
    const int64_t *row = out.nodes.data() + static_cast<size_t>(kNodeWords) * r;
    int64_t *c = out.cracks.data() + static_cast<size_t>(kCrackWords) * static_cast<size_t>(row[0]);
    c[0] += 1;
    if (row[9] == 1) c[2] += 1;
    if (row[9] >= 3) c[3] += 1;
    c[5] = std::max(c[5], row[9]);
  }
  for (size_t r = 0; r < cracks; ++r) {
    int64_t *c = out.cracks.data() + static_cast<size_t>(kCrackWords) * r;
    c[4] = c[1] - c[0] + 1;
    if (c[4] < 0) return kBruteLoops;  // (cannot be: the diagram of a connected crack is connected)
  }
  return kBruteOk;
}

}  // namespace cs
}  // namespace pcp
