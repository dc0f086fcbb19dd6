// pcp_crack_branch.hpp -- the arithmetic of the crack branches on the map ("Crack branches on the map", CB1-CB9),
// one copy for the device stage (pcp_crack_branch.hip: its graph part runs on the host), the CPU form (pcp_crack_branches_host)
// and the host self-test (host/crack_branch_selftest.cpp): the limits of `prune`, the decomposition of a node set into
// branches, junctions and bridges, the one round of spur pruning, the graph words of the tables, CB8's lengths, and the whole
// stage by brute force on cs::skeleton_brute.  Every result but CB8's doubles is an integer that has one value whatever
// computes it.  Host only but for the two functions of CB1.  Build without floating-point contraction.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "pcp_crack_direction.hpp"
#include "pcp_crack_skeleton.hpp"

namespace pcp {
namespace cb {

constexpr int kRowWords = 15;    // CB5: crack_row nodes edges_inside attachments junction_u junction_v points sum_w min_w max_w
                                 //      pos_min pos_max sum_qx sum_qy sum_qz
constexpr int kGraphWords = 6;   // ... of which the host fills the first six
constexpr int kCrackWords = 7;   // CB7: branches bridges junctions_kept ends_kept pruned_branches pruned_nodes pruned_points
constexpr float kMaxPrune = 1024.0f;  // CB1
// CB4 (per point and per node) and CB7 (per edge)
constexpr int32_t kNoPoint = -1, kJunction = -2, kPruned = -3;
constexpr int32_t kBridge = -1, kEdgePruned = -2;

// ---- CB1 (a NaN fails the first comparison; the product is exact in fp64 and at most 2^30) ----------------------------------
PCP_CF_HD bool prune_ok(float prune) { return prune >= 0.0f && prune <= kMaxPrune; }
PCP_CF_HD uint64_t prune_q_of(float prune) { return static_cast<uint64_t>(static_cast<double>(prune) * 1048576.0); }

// ---- CB2: the decomposition of the node set keep[] (N node rows, E ordered edges u v links) ---------------------------------
struct Parts {
  std::vector<int32_t> degree;  // N: deg_K, 0 outside K
  std::vector<int32_t> of;      // N: the lowest node row of the node's branch; kJunction; kPruned outside K
  std::vector<int32_t> heads;   // the branches: their lowest node rows, ascending
};

inline void decompose(int64_t N, const int64_t *edges, int64_t E, const std::vector<uint8_t> &keep, Parts &out) {
  const size_t sn = static_cast<size_t>(N);
  out.degree.assign(sn, 0);
  auto inside = [&](int64_t e) { return keep[static_cast<size_t>(edges[3 * e])] && keep[static_cast<size_t>(edges[3 * e + 1])]; };
  for (int64_t e = 0; e < E; ++e)
    if (inside(e)) {
      out.degree[static_cast<size_t>(edges[3 * e])] += 1;
      out.degree[static_cast<size_t>(edges[3 * e + 1])] += 1;
    }
  // a union-find over the non-junction nodes whose roots are the lowest rows
  std::vector<int32_t> parent(sn);
  for (size_t v = 0; v < sn; ++v) parent[v] = static_cast<int32_t>(v);
  auto find = [&](int32_t v) {
    while (parent[static_cast<size_t>(v)] != v) {
      parent[static_cast<size_t>(v)] = parent[static_cast<size_t>(parent[static_cast<size_t>(v)])];
      v = parent[static_cast<size_t>(v)];
    }
    return v;
  };
  for (int64_t e = 0; e < E; ++e) {
    if (!inside(e)) continue;
    const int32_t u = static_cast<int32_t>(edges[3 * e]), v = static_cast<int32_t>(edges[3 * e + 1]);
    if (out.degree[static_cast<size_t>(u)] >= 3 || out.degree[static_cast<size_t>(v)] >= 3) continue;
    const int32_t ru = find(u), rv = find(v);
    if (ru < rv) parent[static_cast<size_t>(rv)] = ru;
    if (rv < ru) parent[static_cast<size_t>(ru)] = rv;
  }
  out.of.assign(sn, kPruned);
  out.heads.clear();
  for (size_t v = 0; v < sn; ++v) {
    if (!keep[v]) continue;
    if (out.degree[v] >= 3) {
      out.of[v] = kJunction;
      continue;
    }
    out.of[v] = find(static_cast<int32_t>(v));
    if (out.of[v] == static_cast<int32_t>(v)) out.heads.push_back(static_cast<int32_t>(v));
  }
}

// ---- CB2-CB7: the graph part -----------------------------------------------------------------------------------------------
struct Graph {
  std::vector<int32_t> node_branch;  // N: the branch row, kJunction or kPruned
  std::vector<int32_t> heads;        // B: the lowest node row of every final branch (its id is that node's id)
  std::vector<int64_t> rows;         // 15 B: the graph words filled, the point words zero
  std::vector<int32_t> edge_branch;  // E
  std::vector<int64_t> cracks;       // 7 C
  int64_t pruned_branches = 0;
};

// node_crack, node_points: N (CS4's crack_row and points); ends: 2 C, the node rows of node[end_a], node[end_b] (CL7)
inline void graph(int64_t N, const int64_t *node_crack, const int64_t *node_points, const int64_t *edges, int64_t E, int64_t C,
                  const int32_t *ends, uint64_t step_q, uint64_t prune_q, Graph &out) {
  const size_t sn = static_cast<size_t>(N), se = static_cast<size_t>(E), sc = static_cast<size_t>(C);
  // CB3: the whole diagram, its spurs, one round
  std::vector<uint8_t> keep(sn, 1);
  Parts all;
  decompose(N, edges, E, keep, all);
  std::vector<int64_t> count(sn, 0), attached(sn, 0);  // per head
  std::vector<uint8_t> holds_end(sn, 0);
  for (size_t v = 0; v < sn; ++v)
    if (all.of[v] >= 0) count[static_cast<size_t>(all.of[v])] += 1;
  for (size_t r = 0; r < 2 * sc; ++r) {
    const int32_t b = all.of[static_cast<size_t>(ends[r])];
    if (b >= 0) holds_end[static_cast<size_t>(b)] = 1;
  }
  for (int64_t e = 0; e < E; ++e) {
    const int32_t bu = all.of[static_cast<size_t>(edges[3 * e])], bv = all.of[static_cast<size_t>(edges[3 * e + 1])];
    if (bu >= 0 && bv == kJunction) attached[static_cast<size_t>(bu)] += 1;
    if (bv >= 0 && bu == kJunction) attached[static_cast<size_t>(bv)] += 1;
  }
  out.cracks.assign(static_cast<size_t>(kCrackWords) * sc, 0);
  out.pruned_branches = 0;
  std::vector<uint8_t> spur(sn, 0);
  for (int32_t h : all.heads) {
    const size_t sh = static_cast<size_t>(h);
    spur[sh] = attached[sh] == 1 && !holds_end[sh] && static_cast<uint64_t>(count[sh]) * step_q < prune_q;
    if (!spur[sh]) continue;
    out.pruned_branches += 1;
    out.cracks[kCrackWords * static_cast<size_t>(node_crack[sh]) + 4] += 1;
  }
  for (size_t v = 0; v < sn; ++v)
    if (all.of[v] >= 0 && spur[static_cast<size_t>(all.of[v])]) {
      keep[v] = 0;
      int64_t *c = out.cracks.data() + kCrackWords * static_cast<size_t>(node_crack[v]);
      c[5] += 1;
      c[6] += node_points[v];
    }
  // the final branches: the decomposition of what is kept
  Parts kept;
  decompose(N, edges, E, keep, kept);
  out.heads = kept.heads;
  const size_t sb = out.heads.size();
  std::vector<int32_t> row_of_head(sn, -1);
  for (size_t b = 0; b < sb; ++b) row_of_head[static_cast<size_t>(out.heads[b])] = static_cast<int32_t>(b);
  out.node_branch.assign(sn, kPruned);
  out.rows.assign(static_cast<size_t>(kRowWords) * sb, 0);
  for (size_t b = 0; b < sb; ++b) {
    int64_t *row = out.rows.data() + kRowWords * b;
    row[0] = node_crack[static_cast<size_t>(out.heads[b])];
    row[4] = row[5] = -1;
    out.cracks[kCrackWords * static_cast<size_t>(row[0])] += 1;
  }
  for (size_t v = 0; v < sn; ++v) {
    if (!keep[v]) continue;
    int64_t *c = out.cracks.data() + kCrackWords * static_cast<size_t>(node_crack[v]);
    if (kept.degree[v] == 1) c[3] += 1;
    if (kept.of[v] == kJunction) {
      out.node_branch[v] = kJunction;
      c[2] += 1;
      continue;
    }
    out.node_branch[v] = row_of_head[static_cast<size_t>(kept.of[v])];
    out.rows[kRowWords * static_cast<size_t>(out.node_branch[v]) + 1] += 1;
  }
  // CB7 per edge, and with it CB5's edges_inside, attachments and junctions (the edges ascend by (u, v): the lower junction
  // row of a branch with two comes first unless its second attachment has the lower one, which the swap below settles)
  out.edge_branch.assign(se, kEdgePruned);
  for (size_t e = 0; e < se; ++e) {
    const size_t u = static_cast<size_t>(edges[3 * e]), v = static_cast<size_t>(edges[3 * e + 1]);
    if (!keep[u] || !keep[v]) continue;
    const int32_t bu = out.node_branch[u], bv = out.node_branch[v];
    if (bu == kJunction && bv == kJunction) {
      out.edge_branch[e] = kBridge;
      out.cracks[kCrackWords * static_cast<size_t>(node_crack[u]) + 1] += 1;
      continue;
    }
    const int32_t b = bu >= 0 ? bu : bv;
    out.edge_branch[e] = b;
    int64_t *row = out.rows.data() + kRowWords * static_cast<size_t>(b);
    if (bu >= 0 && bv >= 0) {
      row[2] += 1;
      continue;
    }
    const int64_t junction = static_cast<int64_t>(bu >= 0 ? v : u);
    row[3] += 1;
    if (row[4] < 0) {
      row[4] = junction;
    } else {
      row[5] = junction;
      if (row[5] < row[4]) std::swap(row[4], row[5]);
    }
  }
}

// ---- CB8: host arithmetic on the integers (cs::centroid per axis, the edge lengths of CS7) ------------------------------------
inline double edge_length(const int64_t *nodes10, int64_t u, int64_t v) {
  double d[3];
  for (int a = 0; a < 3; ++a)
    d[a] = cs::centroid(nodes10[cs::kNodeWords * v + 6 + a], nodes10[cs::kNodeWords * v + 2]) -
           cs::centroid(nodes10[cs::kNodeWords * u + 6 + a], nodes10[cs::kNodeWords * u + 2]);
  return std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// length_m (B) and kept_length_m (C), zeroed here: the sums in edge-row order, one addition after the other
inline void lengths(const int64_t *nodes10, const int64_t *edges, const int32_t *edge_branch, int64_t E, int64_t B, int64_t C,
                    double *length_m, double *kept_length_m) {
  std::fill(length_m, length_m + B, 0.0);
  std::fill(kept_length_m, kept_length_m + C, 0.0);
  for (int64_t e = 0; e < E; ++e) {
    if (edge_branch[e] < kBridge) continue;
    const double l = edge_length(nodes10, edges[3 * e], edges[3 * e + 1]);
    if (edge_branch[e] >= 0) length_m[edge_branch[e]] += l;
    kept_length_m[nodes10[cs::kNodeWords * edges[3 * e]]] += l;
  }
}

// ---- the whole stage on the host (the core of pcp_crack_branches_host) ------------------------------------------------------
struct HostResult {
  std::vector<int32_t> branch;       // n
  std::vector<int32_t> ids;          // B
  std::vector<int64_t> rows;         // 15 B
  std::vector<int64_t> moments;      // 20 B
  std::vector<int32_t> edge_branch;  // E
  std::vector<int64_t> cracks;       // 7 C
  int64_t pruned_branches = 0;
};

enum Brute { kBruteOk = 0, kBruteRange = 1, kBruteLoops = 2, kBruteLinks = 3 };

// xyz: n x 3; views, sum_q (nullable: every fused width 0): n.  Quadratic in the crack points.
inline Brute branches_brute(int64_t n, const float *xyz, const uint32_t *views, const uint64_t *sum_q, int32_t min_views, float t,
                            uint64_t step_q, uint64_t prune_q, HostResult &out) {
  const size_t sn = static_cast<size_t>(n);
  cs::HostResult sk;
  cl::HostResult len;
  const cs::Brute how = cs::skeleton_brute(n, xyz, views, sum_q, min_views, t, step_q, sk, &len);  // CB1
  if (how != cs::kBruteOk) return how == cs::kBruteRange ? kBruteRange : kBruteLoops;
  const size_t N = sk.ids.size(), E = sk.edges.size() / cs::kEdgeWords, C = sk.cracks.size() / cs::kCrackWords;
  std::vector<int32_t> row_of_id(sn, -1);
  for (size_t r = 0; r < N; ++r) row_of_id[static_cast<size_t>(sk.ids[r])] = static_cast<int32_t>(r);
  auto node_row = [&](int64_t i) { return row_of_id[static_cast<size_t>(sk.node[static_cast<size_t>(i)])]; };
  std::vector<int64_t> node_crack(N), node_points(N);
  for (size_t r = 0; r < N; ++r) node_crack[r] = sk.nodes[cs::kNodeWords * r], node_points[r] = sk.nodes[cs::kNodeWords * r + 2];
  std::vector<int32_t> ends(2 * C);
  for (size_t r = 0; r < C; ++r) {
    ends[2 * r] = node_row(len.rows[cl::kRowWords * r]);
    ends[2 * r + 1] = node_row(len.rows[cl::kRowWords * r + 1]);
  }
  Graph g;
  graph(static_cast<int64_t>(N), node_crack.data(), node_points.data(), sk.edges.data(), static_cast<int64_t>(E), static_cast<int64_t>(C),
        ends.data(), step_q, prune_q, g);
  const size_t B = g.heads.size();
  out.ids.resize(B);
  for (size_t b = 0; b < B; ++b) out.ids[b] = sk.ids[static_cast<size_t>(g.heads[b])];
  out.rows = g.rows;
  out.edge_branch = g.edge_branch;
  out.cracks = g.cracks;
  out.pruned_branches = g.pruned_branches;
  out.branch.assign(sn, kNoPoint);
  out.moments.assign(static_cast<size_t>(cd::kRowWords) * B, 0);
  for (size_t b = 0; b < B; ++b) out.rows[kRowWords * b + 8] = INT64_MAX, out.rows[kRowWords * b + 10] = INT64_MAX;
  std::vector<int32_t> list;
  std::vector<int32_t> brow(sn, kNoPoint);  // the branch ROW per point
  for (int64_t i = 0; i < n; ++i) {
    const size_t si = static_cast<size_t>(i);
    if (sk.node[si] < 0) continue;
    const int32_t b = g.node_branch[static_cast<size_t>(node_row(i))];
    brow[si] = b;
    out.branch[si] = b >= 0 ? out.ids[static_cast<size_t>(b)] : b;  // CB4
    if (b < 0) continue;
    list.push_back(static_cast<int32_t>(i));
    int64_t *row = out.rows.data() + kRowWords * static_cast<size_t>(b);  // CB5
    const int64_t w = sum_q ? static_cast<int64_t>(cf::fused_w(sum_q[si], views[si])) : 0;
    const int64_t pos = static_cast<int64_t>(len.pos[si]);
    row[6] += 1;
    row[7] += w;
    row[8] = std::min(row[8], w);
    row[9] = std::max(row[9], w);
    row[10] = std::min(row[10], pos);
    row[11] = std::max(row[11], pos);
    for (int a = 0; a < 3; ++a) row[12 + a] += cs::quant(xyz[3 * si + a]);
  }
  for (size_t a = 0; a < list.size(); ++a) {  // CB6
    const size_t i = static_cast<size_t>(list[a]);
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    gn::Moments mo;
    gn::clear(mo);
    for (size_t b = 0; b < list.size(); ++b) {
      const size_t j = static_cast<size_t>(list[b]);
      if (b == a || brow[j] != brow[i]) continue;
      gn::visit(mo, xyz[3 * j] - x, xyz[3 * j + 1] - y, xyz[3 * j + 2] - z, t);
    }
    if (mo.n >= gn::kMaxNeighbours) return kBruteLinks;
    int64_t w[gn::kMomentWords];
    gn::store(mo, w);
    int64_t *row = out.moments.data() + static_cast<size_t>(cd::kRowWords) * static_cast<size_t>(brow[i]);
    for (int k = 0; k < gn::kMomentWords; ++k) {
      row[2 * k] = static_cast<int64_t>(static_cast<uint64_t>(row[2 * k]) + cd::lo_of(w[k]));
      row[2 * k + 1] += cd::hi_of(w[k]);
    }
  }
  return kBruteOk;
}

}  // namespace cb
}  // namespace pcp
