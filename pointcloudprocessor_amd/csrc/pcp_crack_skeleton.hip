// pcp_crack_skeleton.hip -- crack skeletons on the map ("Crack skeletons on the map", CS1-CS9): the level-set
// diagram of every crack of pcp_crack_components under the arc positions of pcp_crack_lengths -- its branches, junctions and
// loops.  The reference's script gets as far as a 2-D skeleton per keyframe (pcv.morphology.skeletonize in preprocess() of
// scripts/genNormAndDistanceMask.py).
//
// The stage runs after the length stage for its parameters (crack_map_run, pcp_crack_fuse.hip) on that call's scratch:
// D_a, the crack's row and the grid, all indexed by the PLACE of a crack point in the cell order.  A band kernel cuts the
// cracks at equal steps of D_a; the component stage's union walk, restricted to links inside a band, makes the nodes
// (flatten, scan, ids as there); a statistics kernel fills one row per node with integer atomics, merged per wavefront where
// its lanes share a node; the same walk once more puts every link between two nodes into a hash set of edges by
// compare-and-swap and counts it there.  A full set raises a flag and the host reruns the walk on a set twice as large, a
// bounded number of times.  The occupied slots are compacted and ordered on the host (they are of the order of the nodes);
// degrees and the per-crack summary are integer atomics over the unique edges and the nodes.  No lane waits for another one
// and no kernel loops on a word that another workgroup writes.
#include <algorithm>
#include <cstdlib>
#include <new>
#include <vector>

#include "pcp_device.hpp"
#include "pcp_crack_map.hpp"
#include "pcp_scan.hpp"
#include "pcp_crack_skeleton.hpp"

namespace pcp {

constexpr int kCsBlock = 256;
constexpr int kCsMinSetLog2 = 6, kCsMaxSetLog2 = 31;  // (the tests start at the smallest set to walk the growth)
constexpr int kCsMaxDoublings = 12;                   // CS8: reruns of the edge walk before PCP_ERR_NOMEM
constexpr uint32_t kCsMaxProbes = 1024;               // linear probes before a lane asks for a larger set
// words of the call's flags: the set is full; something that cannot be; the unique edges; the cursor of the compaction
enum { CS_FULL = 0, CS_BAD = 1, CS_EDGES = 2, CS_CURSOR = 3, CS_WORDS = 4 };

static inline uint32_t cs_blocks(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kCsBlock))); }

// CS8: words that other lanes may change in the same kernel are read at agent scope (CC5, CL8)
__device__ __forceinline__ unsigned long long cs_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t cs_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// CS2 per place, and every point its own node to begin with (parent is indexed by view index, as CC5's)
__global__ __launch_bounds__(kCsBlock) void k_cs_band(const unsigned long long *__restrict__ dist, int64_t m, unsigned long long step_q,
                                                      int32_t *__restrict__ band, int32_t *__restrict__ parent) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  if (s >= m) return;
  band[s] = static_cast<int32_t>(cs::band(dist[s], step_q));  // (pos <= (m - 1) w_max and step_q >= w_max: below m)
  parent[s] = static_cast<int32_t>(s);
}

// CS3: k_cc_union's walk (one lane per place, the candidates the places after it, every pair once) over the links that
// stay inside a band
__global__ __launch_bounds__(kCsBlock) void k_cs_union(const float *__restrict__ gx, const float *__restrict__ gy,
                                                       const float *__restrict__ gz, const int32_t *__restrict__ order,
                                                       const int32_t *__restrict__ band, int64_t m, GridDesc g,
                                                       const int32_t *__restrict__ start, float t, int32_t *__restrict__ parent) {
  const int64_t s64 = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  if (s64 >= m) return;
  const int32_t s = static_cast<int32_t>(s64);
  const float qx = gx[s], qy = gy[s], qz = gz[s];
  const int32_t mine = order[s], my_band = band[s];
  crack_walk<true>(g, start, qx, qy, qz, s, m, [&](int32_t c) {
    if (band[c] == my_band && cl::d2_of(gx[c] - qx, gy[c] - qy, gz[c] - qz) <= t) cc_unite(parent, mine, order[c]);
  });
}

// one lane per view index k (rank[k] = roots before k: the rows ascend by id because the list does): the row of k's node by
// place, node[] by input index, and for a root the id and the empty row with the crack's row and the band
__global__ __launch_bounds__(kCsBlock) void k_cs_ids(const int32_t *__restrict__ root_of, const int32_t *__restrict__ rank,
                                                     const int32_t *__restrict__ list, const int32_t *__restrict__ place_of,
                                                     const int32_t *__restrict__ row_of, const int32_t *__restrict__ band, int64_t m,
                                                     int32_t *__restrict__ node_row, int32_t *__restrict__ node /* nullable */,
                                                     int32_t *__restrict__ ids, unsigned long long *__restrict__ table) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  if (k >= m) return;
  const int32_t root = root_of[k], r = rank[root], s = place_of[k];
  node_row[s] = r;
  if (node) node[list[k]] = list[root];
  if (root != static_cast<int32_t>(k)) return;
  ids[r] = list[k];
  unsigned long long *row = table + static_cast<int64_t>(cs::kNodeWords) * r;
  row[0] = static_cast<unsigned long long>(row_of[s]);
  row[1] = static_cast<unsigned long long>(band[s]);
#pragma unroll
  for (int w = 2; w < cs::kNodeWords; ++w) row[w] = 0;
  row[4] = ~0ull;  // min_w
}

// CS4: one lane per place (neighbours in space are neighbours in the wavefront, and mostly of one node): where all the lanes
// of a wavefront share a node their values are merged first and one lane issues the atomics.  The sums of the coordinates'
// quanta are signed: two's complement sums in unsigned words.
__global__ __launch_bounds__(kCsBlock) void k_cs_nodes(const float *__restrict__ gx, const float *__restrict__ gy,
                                                       const float *__restrict__ gz, const int32_t *__restrict__ order, int64_t m,
                                                       const int32_t *__restrict__ node_row, const int32_t *__restrict__ list, int64_t n,
                                                       const uint32_t *__restrict__ u32, const unsigned long long *__restrict__ u64,
                                                       unsigned long long *__restrict__ table) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  const bool valid = s < m;
  int32_t row = -1;
  unsigned long long points = 0, sum_w = 0, sx = 0, sy = 0, sz = 0;
  uint32_t min_w = 0xffffffffu, max_w = 0;
  if (valid) {
    row = node_row[s];
    const int32_t i = list[order[s]];
    const uint32_t w = cf::fused_w(u64[i], u32[n + i]);
    points = 1;
    sum_w = w;
    min_w = max_w = w;
    sx = static_cast<unsigned long long>(cs::quant(gx[s]));
    sy = static_cast<unsigned long long>(cs::quant(gy[s]));
    sz = static_cast<unsigned long long>(cs::quant(gz[s]));
  }
  bool shared;
  const bool issue = wave_row_issuer(valid, row, &shared);
  if (shared) {
    points = wave_sum_u64(points);
    sum_w = wave_sum_u64(sum_w);
    sx = wave_sum_u64(sx);
    sy = wave_sum_u64(sy);
    sz = wave_sum_u64(sz);
    min_w = wave_min_u32(min_w);
    max_w = wave_max_u32(max_w);
  }
  if (!issue) return;
  unsigned long long *st = table + static_cast<int64_t>(cs::kNodeWords) * row;
  atomicAdd(st + 2, points);
  atomicAdd(st + 3, sum_w);
  atomicMin(st + 4, static_cast<unsigned long long>(min_w));
  atomicMax(st + 5, static_cast<unsigned long long>(max_w));
  atomicAdd(st + 6, sx);
  atomicAdd(st + 7, sy);
  atomicAdd(st + 8, sz);
}

__global__ __launch_bounds__(kCsBlock) void k_cs_set_clear(unsigned long long *__restrict__ keys, uint32_t *__restrict__ links, int64_t slots) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  if (i >= slots) return;
  keys[i] = cs::kNoKey;
  links[i] = 0;
}

__device__ __forceinline__ uint64_t cs_mix(uint64_t x) {  // (splitmix64's finaliser)
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// `count` links of the edge `key` into the set of mask + 1 slots: the slot is found or taken by compare-and-swap within a
// bounded number of probes, or the set is reported full.  Once it is, the other lanes do not probe any more.
__device__ __forceinline__ void cs_add(unsigned long long *keys, uint32_t *links, uint32_t mask, uint64_t key, uint32_t count,
                                       uint32_t *words) {
  if (cs_load(words + CS_FULL)) return;
  const uint32_t probes = min(mask, kCsMaxProbes - 1) + 1;
  uint32_t h = static_cast<uint32_t>(cs_mix(key)) & mask;
  for (uint32_t p = 0; p < probes; ++p, h = (h + 1) & mask) {
    unsigned long long cur = cs_load(keys + h);
    if (cur == cs::kNoKey) {
      cur = atomicCAS(keys + h, static_cast<unsigned long long>(cs::kNoKey), static_cast<unsigned long long>(key));
      if (cur == cs::kNoKey) {
        atomicAdd(words + CS_EDGES, 1u);
        cur = key;
      }
    }
    if (cur == key) {
      atomicAdd(links + h, count);
      return;
    }
  }
  atomicMax(words + CS_FULL, 1u);
}

// CS5: the union kernel's walk once more; a linked pair in two nodes is a link of the edge between them.  A lane keeps its
// last key and the hits on it, and goes to the set when the key changes.
__global__ __launch_bounds__(kCsBlock) void k_cs_edges(const float *__restrict__ gx, const float *__restrict__ gy,
                                                       const float *__restrict__ gz, const int32_t *__restrict__ band,
                                                       const int32_t *__restrict__ node_row, int64_t m, GridDesc g,
                                                       const int32_t *__restrict__ start, float t, unsigned long long *__restrict__ keys,
                                                       uint32_t *__restrict__ links, uint32_t mask, uint32_t *__restrict__ words) {
  const int64_t s64 = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  if (s64 >= m) return;
  const int32_t s = static_cast<int32_t>(s64);
  const float qx = gx[s], qy = gy[s], qz = gz[s];
  const int32_t my_node = node_row[s], my_band = band[s];
  uint64_t last = cs::kNoKey;
  uint32_t hits = 0;
  crack_walk<true>(g, start, qx, qy, qz, s, m, [&](int32_t c) {
    const int32_t other = node_row[c];
    if (other == my_node || !(cl::d2_of(gx[c] - qx, gy[c] - qy, gz[c] - qz) <= t)) return;
    const int32_t its_band = band[c];
    if (its_band != my_band + 1 && my_band != its_band + 1) {  // (cannot be: CS2)
      atomicMax(words + CS_BAD, 1u);
      return;
    }
    const uint64_t key = my_band < its_band ? cs::edge_key(my_node, other) : cs::edge_key(other, my_node);
    if (key == last) {
      ++hits;
      return;
    }
    if (hits) cs_add(keys, links, mask, last, hits, words);
    last = key;
    hits = 1;
  });
  if (hits) cs_add(keys, links, mask, last, hits, words);
}

// the occupied slots, in any order (the host orders them)
__global__ __launch_bounds__(kCsBlock) void k_cs_compact(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ links,
                                                         int64_t slots, int64_t capacity, unsigned long long *__restrict__ out,
                                                         uint32_t *__restrict__ words) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  if (i >= slots) return;
  const unsigned long long key = keys[i];
  if (key == cs::kNoKey) return;
  const uint32_t at = atomicAdd(words + CS_CURSOR, 1u);
  if (at >= capacity) return;  // (cannot be: capacity is the count of the insertions)
  out[2 * static_cast<int64_t>(at)] = key;
  out[2 * static_cast<int64_t>(at) + 1] = links[i];
}

// CS4's degree and CS6's edges, one lane per unique edge
__global__ __launch_bounds__(kCsBlock) void k_cs_degree(const unsigned long long *__restrict__ edges, int64_t count, int64_t node_rows,
                                                        int64_t crack_rows, unsigned long long *__restrict__ table,
                                                        unsigned long long *__restrict__ cracks, uint32_t *__restrict__ words) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  if (i >= count) return;
  const unsigned long long key = edges[2 * i];
  const int64_t u = cs::key_u(key), v = cs::key_v(key);
  if (u < 0 || u >= node_rows || v < 0 || v >= node_rows) {  // (cannot be)
    atomicMax(words + CS_BAD, 1u);
    return;
  }
  atomicAdd(table + cs::kNodeWords * u + 9, 1ull);
  atomicAdd(table + cs::kNodeWords * v + 9, 1ull);
  const unsigned long long r = table[cs::kNodeWords * u];  // (written by an earlier kernel)
  if (r >= static_cast<unsigned long long>(crack_rows)) {
    atomicMax(words + CS_BAD, 1u);
    return;
  }
  atomicAdd(cracks + cs::kCrackWords * r + 1, 1ull);
}

// CS6, one lane per node, after the degrees are final
__global__ __launch_bounds__(kCsBlock) void k_cs_summary(const unsigned long long *__restrict__ table, int64_t node_rows, int64_t crack_rows,
                                                         unsigned long long *__restrict__ cracks, uint32_t *__restrict__ words) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  if (i >= node_rows) return;
  const unsigned long long r = table[cs::kNodeWords * i], degree = table[cs::kNodeWords * i + 9];
  if (r >= static_cast<unsigned long long>(crack_rows)) {  // (cannot be)
    atomicMax(words + CS_BAD, 1u);
    return;
  }
  unsigned long long *c = cracks + cs::kCrackWords * r;
  atomicAdd(c + 0, 1ull);
  if (degree == 1) atomicAdd(c + 2, 1ull);
  if (degree >= 3) atomicAdd(c + 3, 1ull);
  if (degree > 0) atomicMax(c + 5, degree);
}

// CS6: loops = edges - nodes + 1 >= 0, asserted
__global__ __launch_bounds__(kCsBlock) void k_cs_loops(unsigned long long *__restrict__ cracks, int64_t crack_rows, uint32_t *__restrict__ words) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kCsBlock + threadIdx.x;
  if (r >= crack_rows) return;
  unsigned long long *c = cracks + cs::kCrackWords * r;
  if (c[0] < 1 || c[1] + 1 < c[0]) {
    atomicMax(words + CS_BAD, 1u);
    return;
  }
  c[4] = c[1] + 1 - c[0];
}

hipError_t preload_crack_skeleton() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_cs_edges));
}

// a compacted slot of the edge set, as k_cs_compact writes it
struct CsRec {
  unsigned long long key, links;
};
static_assert(sizeof(CsRec) == 16, "two words per compacted edge");

static int64_t first_slots(int64_t node_rows) {
  int log2 = kCsMinSetLog2;
  while (log2 < kCsMaxSetLog2 && (int64_t(1) << log2) < 4 * node_rows) ++log2;  // (edges are of the order of the nodes)
  if (const char *e = std::getenv("PCP_SKELETON_SET_LOG2"))  // read per call: the tests shrink the set inside one process
    log2 = std::min(kCsMaxSetLog2, std::max(kCsMinSetLog2, std::atoi(e)));
  return int64_t(1) << log2;
}

// the m > 0 crack points and rows > 0 cracks the length stage left in cc, cl and ctx->g_*
int crack_skeleton_run(pcp_context *ctx, const pcp_crack_link_params &p, uint64_t step_q, const CcScratch &cc, const ClScratch &cl, CsScratch &s,
                       CrackCounts *c) {
  CrackMap &cm = *ctx->crack;
  const int64_t m = c->points, rows = c->cracks;
  float largest = 0.0f;
  for (int a = 0; a < 3; ++a) largest = std::max(largest, std::max(fabsf(cc.lo[a]), fabsf(cc.hi[a])));
  if (!cs::coord_ok(largest) || !cs::sums_fit(m, largest))  // CS4
    return set_error(ctx, PCP_ERR_RANGE, "pcp_crack_skeleton: a crack point has a coordinate of %g m (beyond 2^20 m, or too large for exact sums over %lld points)",
                     static_cast<double>(largest), (long long)m);
  const size_t sm = static_cast<size_t>(m), sr = static_cast<size_t>(rows);
  const size_t pm = (sm + 3) & ~size_t(3);
  const float *gx = ctx->g_xyz.p, *gy = ctx->g_xyz.p + pm, *gz = ctx->g_xyz.p + 2 * pm;
  const float t = gn::threshold_of(p.radius);
  for (DevBuf<int32_t> *b : {&s.band, &s.parent, &s.root_of, &s.node_row}) PCP_HIP_TRY(ctx, b->ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.rank.ensure(sm + 8));
  PCP_HIP_TRY(ctx, s.words.ensure(CS_WORDS));
  PCP_HIP_TRY(ctx, cm.cs_cracks.ensure(static_cast<size_t>(cs::kCrackWords) * sr + 4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.rank.p, 0, (sm + 8) * 4, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.words.p, 0, CS_WORDS * 4, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(cm.cs_cracks.p, 0, cs::kCrackWords * sr * 8, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cs_band, dim3(cs_blocks(m)), dim3(kCsBlock), 0, ctx->stream, cl.dist.p, m, static_cast<unsigned long long>(step_q),
                       s.band.p, s.parent.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cs_union, dim3(cs_blocks(m)), dim3(kCsBlock), 0, ctx->stream, gx, gy, gz, ctx->g_order.p, s.band.p, m, cc.grid,
                       ctx->g_start.p, t, s.parent.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  int64_t nodes = 0;
  int rc = crack_label_forest(ctx, "pcp_crack_skeleton", "nodes", s.parent.p, nullptr, m, rows, s.root_of.p, s.rank.p, nullptr, &nodes);
  if (rc != PCP_OK) return rc;
  const size_t sk = static_cast<size_t>(nodes);
  PCP_HIP_TRY(ctx, cm.cs_ids.ensure(sk + 4));
  PCP_HIP_TRY(ctx, cm.cs_nodes.ensure(static_cast<size_t>(cs::kNodeWords) * sk + 4));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cs_ids, dim3(cs_blocks(m)), dim3(kCsBlock), 0, ctx->stream, s.root_of.p, s.rank.p, cc.list.p, cl.place_of.p, cl.row_of.p,
                       s.band.p, m, s.node_row.p, s.node.p, cm.cs_ids.p, cm.cs_nodes.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cs_nodes, dim3(cs_blocks(m)), dim3(kCsBlock), 0, ctx->stream, gx, gy, gz, ctx->g_order.p, m, s.node_row.p, cc.list.p,
                       ctx->n, cm.cf_u32.p, cm.cf_u64.p, cm.cs_nodes.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  // CS8: the edge walk on a set sized from the nodes; a full set is doubled and the walk run again
  int64_t slots = first_slots(nodes);
  uint32_t words[CS_WORDS] = {0, 0, 0, 0};
  int doublings = 0;
  for (;; ++doublings) {
    PCP_HIP_TRY(ctx, s.keys.ensure(static_cast<size_t>(slots)));
    PCP_HIP_TRY(ctx, s.links.ensure(static_cast<size_t>(slots)));
    PCP_HIP_TRY(ctx, hipMemsetAsync(s.words.p, 0, CS_WORDS * 4, ctx->stream));
    {
      LaunchTimer lt(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_cs_set_clear, dim3(cs_blocks(slots)), dim3(kCsBlock), 0, ctx->stream, s.keys.p, s.links.p, slots);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    {
      LaunchTimer lt(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_cs_edges, dim3(cs_blocks(m)), dim3(kCsBlock), 0, ctx->stream, gx, gy, gz, s.band.p, s.node_row.p, m, cc.grid,
                         ctx->g_start.p, t, s.keys.p, s.links.p, static_cast<uint32_t>(slots - 1), s.words.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    PCP_HIP_TRY(ctx, hipMemcpyAsync(words, s.words.p, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (words[CS_BAD]) return set_error(ctx, PCP_ERR_DEVICE, "pcp_crack_skeleton: a link joins bands that are not neighbours");
    if (!words[CS_FULL]) break;
    if (doublings == kCsMaxDoublings || slots >= (int64_t(1) << kCsMaxSetLog2))
      return set_error(ctx, PCP_ERR_NOMEM, "pcp_crack_skeleton: the edge set of %lld slots is full after %d doublings (%lld nodes)", (long long)slots,
                       doublings, (long long)nodes);
    slots *= 2;
  }
  const int64_t edges = words[CS_EDGES];
  std::vector<CsRec> rec;
  try {
    rec.resize(static_cast<size_t>(edges));
    cm.cs_edges.resize(static_cast<size_t>(cs::kEdgeWords) * static_cast<size_t>(edges));
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_crack_skeleton: out of host memory for %lld edges", (long long)edges);
  }
  PCP_HIP_TRY(ctx, s.edges.ensure(2 * static_cast<size_t>(edges) + 4));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    if (edges > 0) {
      hipLaunchKernelGGL(k_cs_compact, dim3(cs_blocks(slots)), dim3(kCsBlock), 0, ctx->stream, s.keys.p, s.links.p, slots, edges, s.edges.p,
                         s.words.p);
      hipLaunchKernelGGL(k_cs_degree, dim3(cs_blocks(edges)), dim3(kCsBlock), 0, ctx->stream, s.edges.p, edges, nodes, rows, cm.cs_nodes.p,
                         cm.cs_cracks.p, s.words.p);
    }
    hipLaunchKernelGGL(k_cs_summary, dim3(cs_blocks(nodes)), dim3(kCsBlock), 0, ctx->stream, cm.cs_nodes.p, nodes, rows, cm.cs_cracks.p,
                       s.words.p);
    hipLaunchKernelGGL(k_cs_loops, dim3(cs_blocks(rows)), dim3(kCsBlock), 0, ctx->stream, cm.cs_cracks.p, rows, s.words.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  if (edges > 0) PCP_HIP_TRY(ctx, hipMemcpyAsync(rec.data(), s.edges.p, 16 * static_cast<size_t>(edges), hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(words, s.words.p, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (words[CS_BAD] || words[CS_CURSOR] != static_cast<uint32_t>(edges))
    return set_error(ctx, PCP_ERR_DEVICE, "pcp_crack_skeleton: %u of %lld edges compacted, flag %u (a crack's diagram is not connected, or a row is out of range)",
                     words[CS_CURSOR], (long long)edges, words[CS_BAD]);
  // CS5: the rows ascend by (u, v) -- the keys order as the pairs do, and they are unique
  std::sort(rec.begin(), rec.end(), [](const CsRec &a, const CsRec &b) { return a.key < b.key; });
  for (size_t e = 0; e < rec.size(); ++e) {
    cm.cs_edges[3 * e] = cs::key_u(rec[e].key);
    cm.cs_edges[3 * e + 1] = cs::key_v(rec[e].key);
    cm.cs_edges[3 * e + 2] = static_cast<int64_t>(rec[e].links);
  }
  c->nodes = nodes;
  c->edges = edges;
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_crack_skeleton(pcp_context *ctx, const pcp_crack_link_params *p, float step, int32_t *out_node, int64_t *out_nodes, int64_t *out_edges) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_nodes) *out_nodes = 0;
  if (out_edges) *out_edges = 0;
  int rc = crack_link_check(ctx, "pcp_crack_skeleton", p);
  if (rc != PCP_OK) return rc;
  const float t = gn::threshold_of(p->radius);
  if (!cs::step_ok(step, t))
    return set_error(ctx, PCP_ERR_INVALID, "pcp_crack_skeleton: step %g outside [%g, 16] (the longest link of radius %g)", static_cast<double>(step),
                     static_cast<double>(cs::w_max_of(t)) * cl::kMetresPerUnit, static_cast<double>(p->radius));
  CrackOut out;
  out.node = out_node;
  CrackCounts c;
  if ((rc = crack_map_run(ctx, *p, CrackMap::kSkeleton, cs::step_q_of(step), out, &c)) != PCP_OK) return rc;
  if (out_nodes) *out_nodes = c.nodes;
  if (out_edges) *out_edges = c.edges;
  return PCP_OK;
}

int pcp_crack_skeleton_nodes_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows10, int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  int64_t rows = 0;
  const int rc = crack_window(ctx, "pcp_crack_skeleton_nodes_fetch", CrackMap::kSkeleton, first, max_rows, ctx->crack->cs_node_rows, &rows);
  if (rc != PCP_OK || rows == 0) return rc;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sr = static_cast<size_t>(rows), sf = static_cast<size_t>(first);
  if (out_id) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_id, ctx->crack->cs_ids.p + sf, sr * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_rows10)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rows10, ctx->crack->cs_nodes.p + cs::kNodeWords * sf, cs::kNodeWords * sr * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_crack_skeleton_edges_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int64_t *out_rows3, int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  int64_t rows = 0;
  const int rc = crack_window(ctx, "pcp_crack_skeleton_edges_fetch", CrackMap::kSkeleton, first, max_rows, static_cast<int64_t>(ctx->crack->cs_edges.size() / cs::kEdgeWords), &rows);
  if (rc != PCP_OK || rows == 0) return rc;
  if (out_rows3) std::copy(ctx->crack->cs_edges.begin() + cs::kEdgeWords * first, ctx->crack->cs_edges.begin() + cs::kEdgeWords * (first + rows), out_rows3);
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_crack_skeleton_cracks_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int64_t *out_rows6, int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  int64_t rows = 0;
  const int rc = crack_window(ctx, "pcp_crack_skeleton_cracks_fetch", CrackMap::kSkeleton, first, max_rows, ctx->crack->cs_crack_rows, &rows);
  if (rc != PCP_OK || rows == 0) return rc;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sr = static_cast<size_t>(rows), sf = static_cast<size_t>(first);
  if (out_rows6)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rows6, ctx->crack->cs_cracks.p + cs::kCrackWords * sf, cs::kCrackWords * sr * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_crack_skeleton_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, float step, const uint64_t *sum_q,
                            int32_t *out_node, int32_t *out_id, int64_t *out_rows10, int64_t edge_capacity, int64_t *out_rows3,
                            int64_t *out_rows6, int64_t *out_nodes, int64_t *out_edges, int64_t *out_cracks) {
  if (out_nodes) *out_nodes = 0;
  if (out_edges) *out_edges = 0;
  if (out_cracks) *out_cracks = 0;
  if (!cf::min_views_ok(min_views) || !gn::radius_ok(radius)) {
    set_global_error("pcp_crack_skeleton_host: min_views %d outside %d..%d or radius %g outside [0.005, 1]", min_views, cf::kMinViewsLo,
                     cf::kMinViewsHi, static_cast<double>(radius));
    return PCP_ERR_INVALID;
  }
  const float t = gn::threshold_of(radius);
  if (!cs::step_ok(step, t)) {
    set_global_error("pcp_crack_skeleton_host: step %g outside [%g, 16] (the longest link of radius %g)", static_cast<double>(step),
                     static_cast<double>(cs::w_max_of(t)) * cl::kMetresPerUnit, static_cast<double>(radius));
    return PCP_ERR_INVALID;
  }
  if (n < 0 || n > cf::kHostMaxPoints || edge_capacity < 0 || (n > 0 && (!xyz || !views))) {
    set_global_error("pcp_crack_skeleton_host: n outside 0..65536, a negative edge capacity or a missing array");
    return PCP_ERR_INVALID;
  }
  cs::HostResult res;
  cs::Brute how = cs::kBruteOk;
  try {
    how = cs::skeleton_brute(n, xyz, views, sum_q, min_views, t, cs::step_q_of(step), res);
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_crack_skeleton_host: out of host memory for %lld points", static_cast<long long>(n));
    return PCP_ERR_NOMEM;
  }
  if (how == cs::kBruteRange) {
    set_global_error("pcp_crack_skeleton_host: a crack point has a coordinate beyond 2^20 m");
    return PCP_ERR_RANGE;
  }
  if (how != cs::kBruteOk) {
    set_global_error("pcp_crack_skeleton_host: a crack's diagram is not connected");
    return PCP_ERR_DEVICE;
  }
  const int64_t edges = static_cast<int64_t>(res.edges.size() / cs::kEdgeWords);
  if (out_node) std::copy(res.node.begin(), res.node.end(), out_node);
  if (out_id) std::copy(res.ids.begin(), res.ids.end(), out_id);
  if (out_rows10) std::copy(res.nodes.begin(), res.nodes.end(), out_rows10);
  if (out_rows3) std::copy(res.edges.begin(), res.edges.begin() + cs::kEdgeWords * std::min(edges, edge_capacity), out_rows3);
  if (out_rows6) std::copy(res.cracks.begin(), res.cracks.end(), out_rows6);
  if (out_nodes) *out_nodes = static_cast<int64_t>(res.ids.size());
  if (out_edges) *out_edges = edges;
  if (out_cracks) *out_cracks = static_cast<int64_t>(res.cracks.size() / cs::kCrackWords);
  return PCP_OK;
}

}  // extern "C"
