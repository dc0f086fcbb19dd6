// pcp_crack_length.hpp -- the arithmetic of the crack lengths on the map ("Crack lengths on the map", CL1-CL9),
// one copy for the kernels (pcp_crack_length.hip), the CPU form (pcp_crack_lengths_host) and the host self-test
// (host/crack_length_selftest.cpp): the integer weight of a link, the tie rules of the ends and of the predecessor, and the
// whole stage by brute force over the pairs with a plain heap Dijkstra.  Every result is an integer that has one value
// whatever computes it.  Build without floating-point contraction.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <queue>
#include <utility>
#include <vector>

#include "pcp_crack_fuse.hpp"

namespace pcp {
namespace cl {

constexpr uint64_t kNoPos = ~uint64_t(0);  // CL5: pos of a point that is no crack point; D of a point not reached yet
constexpr int kRowWords = 7;               // CL7: end_a end_b length_q hops path_sum_w path_min_w path_max_w
constexpr double kMetresPerUnit = 1.0 / 1048576.0;  // CL2: the unit of a weight is 2^-20 m

// ---- CL2 ------------------------------------------------------------------------------------------------------------------
// the fp32 value CC2 compares with the threshold (cf::linked)
PCP_CF_HD float d2_of(float dx, float dy, float dz) { return (dx * dx + dy * dy) + dz * dz; }

// floor of the square root of k <= 2^40 (any k < 2^62 would do): a floating root seeds it, integer comparisons settle it
PCP_CF_HD uint64_t isqrt(uint64_t k) {
  uint64_t w = static_cast<uint64_t>(sqrt(static_cast<double>(k)));
  while (w * w > k) --w;
  while ((w + 1) * (w + 1) <= k) ++w;
  return w;
}

PCP_CF_HD uint64_t weight_of_k(uint64_t k) {
  const uint64_t w = isqrt(k);
  return w < 1 ? 1 : w;
}

// d2 of a linked pair: 0 <= d2 <= t <= 1, so the product is exact in fp64 and k <= 2^40
PCP_CF_HD uint64_t weight(float d2) {
  return weight_of_k(static_cast<uint64_t>(static_cast<double>(d2) * 1099511627776.0));
}

// ---- CL4: the ordered maximum -- the larger D, then the lower index ---------------------------------------------------------
PCP_CF_HD bool end_better(uint64_t d, int32_t index, uint64_t best_d, int32_t best_index) {
  return d > best_d || (d == best_d && index < best_index);
}

// ---- CL6: j (distance dj, link weight w) is a predecessor of a point at distance di; among those the lowest index wins ------
PCP_CF_HD bool pred_ok(uint64_t dj, uint64_t w, uint64_t di) { return dj < di && dj + w == di; }
PCP_CF_HD bool pred_better(int32_t j, int32_t best) { return best < 0 || j < best; }

// ---- the whole stage on the host (the core of pcp_crack_lengths_host) -----------------------------------------------------
struct HostResult {
  std::vector<uint64_t> pos;     // n
  std::vector<int32_t> ids;      // C
  std::vector<int64_t> rows;     // 7 C
  std::vector<int64_t> offsets;  // C + 1
  std::vector<int32_t> path;     // offsets[C]
};

struct Link {
  int32_t to;  // (position in the list of crack points)
  uint32_t w;
};

// D from source s over the adjacency: a plain binary-heap Dijkstra, stale entries skipped
inline void dijkstra(const std::vector<std::vector<Link>> &adj, int32_t s, std::vector<uint64_t> &d) {
  using Item = std::pair<uint64_t, int32_t>;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
  d[static_cast<size_t>(s)] = 0;
  heap.push({0, s});
  while (!heap.empty()) {
    const Item it = heap.top();
    heap.pop();
    if (it.first != d[static_cast<size_t>(it.second)]) continue;
    for (const Link &l : adj[static_cast<size_t>(it.second)]) {
      const uint64_t nd = it.first + l.w;
      if (nd < d[static_cast<size_t>(l.to)]) {
        d[static_cast<size_t>(l.to)] = nd;
        heap.push({nd, l.to});
      }
    }
  }
}

// xyz: n x 3; views, sum_q (nullable: every fused width 0): n.  Host only; quadratic in the crack points.
inline void lengths_brute(int64_t n, const float *xyz, const uint32_t *views, const uint64_t *sum_q, int32_t min_views, float t,
                          HostResult &out) {
  const size_t sn = static_cast<size_t>(n);
  std::vector<int32_t> label(sn);
  cf::label_brute(n, xyz, views, min_views, t, label.data());
  std::vector<int32_t> list, at(sn, -1);  // crack point k = input point list[k]; at = the inverse
  for (int64_t i = 0; i < n; ++i)
    if (label[static_cast<size_t>(i)] >= 0) {
      at[static_cast<size_t>(i)] = static_cast<int32_t>(list.size());
      list.push_back(static_cast<int32_t>(i));
    }
  const size_t m = list.size();
  std::vector<std::vector<Link>> adj(m);  // CL1 / CL2; the rows ascend by index
  for (size_t a = 0; a < m; ++a) {
    const float *p = xyz + 3 * static_cast<size_t>(list[a]);
    for (size_t b = a + 1; b < m; ++b) {
      const float *q = xyz + 3 * static_cast<size_t>(list[b]);
      const float d2 = d2_of(q[0] - p[0], q[1] - p[1], q[2] - p[2]);
      if (!(d2 <= t)) continue;
      const uint32_t w = static_cast<uint32_t>(weight(d2));
      adj[a].push_back({static_cast<int32_t>(b), w});
      adj[b].push_back({static_cast<int32_t>(a), w});
    }
  }
  for (auto &row : adj) std::sort(row.begin(), row.end(), [](const Link &x, const Link &y) { return x.to < y.to; });
  // the members of every crack, ascending; the cracks ascend by id
  std::vector<int32_t> row_of(m, -1);
  std::vector<std::vector<int32_t>> members;
  out.ids.clear();
  for (size_t k = 0; k < m; ++k)
    if (label[static_cast<size_t>(list[k])] == list[k]) {
      row_of[k] = static_cast<int32_t>(members.size());
      members.emplace_back();
      out.ids.push_back(list[k]);
    }
  for (size_t k = 0; k < m; ++k) {
    const int32_t r = row_of[static_cast<size_t>(at[static_cast<size_t>(label[static_cast<size_t>(list[k])])])];
    members[static_cast<size_t>(r)].push_back(static_cast<int32_t>(k));
  }
  const size_t rows = members.size();
  auto farthest = [&](const std::vector<int32_t> &mem, const std::vector<uint64_t> &d) {
    int32_t best = mem[0];
    for (int32_t k : mem)
      if (end_better(d[static_cast<size_t>(k)], k, d[static_cast<size_t>(best)], best)) best = k;
    return best;
  };
  std::vector<uint64_t> d0(m, kNoPos), da(m, kNoPos);
  out.pos.assign(sn, kNoPos);
  out.rows.assign(static_cast<size_t>(kRowWords) * rows, 0);
  out.offsets.assign(rows + 1, 0);
  out.path.clear();
  std::vector<int32_t> chain;
  for (size_t r = 0; r < rows; ++r) {
    const std::vector<int32_t> &mem = members[r];
    dijkstra(adj, mem[0], d0);  // CL4: s0 is the label, the lowest index
    const int32_t a = farthest(mem, d0);
    dijkstra(adj, a, da);
    const int32_t b = farthest(mem, da);
    for (int32_t k : mem) out.pos[static_cast<size_t>(list[static_cast<size_t>(k)])] = da[static_cast<size_t>(k)];
    chain.clear();
    for (int32_t v = b; v != a;) {  // CL6
      chain.push_back(v);
      int32_t pred = -1;
      for (const Link &l : adj[static_cast<size_t>(v)])
        if (pred_ok(da[static_cast<size_t>(l.to)], l.w, da[static_cast<size_t>(v)]) && pred_better(l.to, pred)) pred = l.to;
      v = pred;  // (one exists: v != a was reached through a link)
    }
    chain.push_back(a);
    uint64_t sum_w = 0, min_w = ~uint64_t(0), max_w = 0;
    for (size_t c = chain.size(); c-- > 0;) {
      const int32_t i = list[static_cast<size_t>(chain[c])];
      out.path.push_back(i);
      const uint64_t w = sum_q ? cf::fused_w(sum_q[i], views[i]) : 0;
      sum_w += w;
      min_w = std::min(min_w, w);
      max_w = std::max(max_w, w);
    }
    int64_t *row = out.rows.data() + static_cast<size_t>(kRowWords) * r;
    row[0] = list[static_cast<size_t>(a)];
    row[1] = list[static_cast<size_t>(b)];
    row[2] = static_cast<int64_t>(da[static_cast<size_t>(b)]);
    row[3] = static_cast<int64_t>(chain.size()) - 1;
    row[4] = static_cast<int64_t>(sum_w);
    row[5] = static_cast<int64_t>(min_w);
    row[6] = static_cast<int64_t>(max_w);
    out.offsets[r + 1] = static_cast<int64_t>(out.path.size());
  }
}

}  // namespace cl
}  // namespace pcp
