// pcp_crack_branch.hip -- crack branches on the map ("Crack branches on the map", CB1-CB9): the level-set diagram
// of pcp_crack_skeleton cut at its junctions into branches, the short spurs pruned by one order-free rule, and one exact integer
// record per branch -- its points, width statistics, arc extent, centroid sums and the link moments from which
// pcp_crack_axis_host takes its axis.  The reference's scripts stop at a 2-D skeleton per keyframe and never take it apart.
//
// The stage runs after the skeleton stage for its parameters (crack_map_run, pcp_crack_fuse.hip) on that call's scratch: the
// node row of every place of the cell order, D_a, the grid, and the ordered edges the skeleton stage left on the host.  The
// diagram is of the order of the nodes, so its decomposition (CB2, CB3 and the graph words of CB5 and CB7) is the sequential
// host code of pcp_crack_branch.hpp, fed by one small download; the host uploads the branch row of every node.  The device
// does what scales with the points and the links, one lane per place: k_cb_assign spreads the rows to the places and to
// branch[], k_cb_branches makes the point words and the moments in one walk over the links (crack_walk<false>, the cost class
// of k_cd_directions) -- merged over the wavefront first where its live lanes share a branch, as the statistics kernels of the
// chain do.  Every sum is a 64-bit integer atomic, so the tables do not depend on the order in which the lanes arrive.  No
// lane waits for another one and no kernel loops on a word that another workgroup writes.
#include <algorithm>
#include <new>
#include <vector>

#include "pcp_device.hpp"
#include "pcp_crack_map.hpp"
#include "pcp_crack_branch.hpp"

namespace pcp {

constexpr int kCbBlock = 256;
enum { CB_OVER = 0, CB_BAD = 1, CB_WORDS = 4 };

static inline uint32_t cb_blocks(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kCbBlock))); }

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(v), o, 64)));
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(v), o, 64)));
  return v;
}

// What the host's graph part reads: (crack_row, points) of every node, then per crack the node rows of node[end_a] and
// node[end_b] (CL7; end_a, end_b are view indices).  One lane per node and per crack.
__global__ __launch_bounds__(kCbBlock) void k_cb_gather(const unsigned long long *__restrict__ nodes, int64_t node_rows,
                                                        const int32_t *__restrict__ end_a, const int32_t *__restrict__ end_b,
                                                        const int32_t *__restrict__ place_of, const int32_t *__restrict__ node_row,
                                                        int64_t crack_rows, int64_t m, long long *__restrict__ out,
                                                        uint32_t *__restrict__ words) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCbBlock + threadIdx.x;
  if (i < node_rows) {
    out[2 * i] = static_cast<long long>(nodes[cs::kNodeWords * i]);
    out[2 * i + 1] = static_cast<long long>(nodes[cs::kNodeWords * i + 2]);
  }
  if (i >= crack_rows) return;
  const int32_t ka = end_a[i], kb = end_b[i];
  long long ra = -1, rb = -1;
  if (ka >= 0 && ka < m && kb >= 0 && kb < m) {
    const int32_t sa = place_of[ka], sb = place_of[kb];
    if (sa >= 0 && sa < m && sb >= 0 && sb < m) ra = node_row[sa], rb = node_row[sb];
  }
  if (ra < 0 || ra >= node_rows || rb < 0 || rb >= node_rows) atomicMax(words + CB_BAD, 1u);  // (cannot be)
  out[2 * node_rows + 2 * i] = ra;
  out[2 * node_rows + 2 * i + 1] = rb;
}

// CB4: the branch row (or -2, -3) of every place from its node's, branch[] in input order, and the id of every branch: the
// id of its lowest node (heads, ascending: the rows ascend by id because the nodes' do)
__global__ __launch_bounds__(kCbBlock) void k_cb_assign(const int32_t *__restrict__ node_row, const int32_t *__restrict__ node_branch,
                                                        const int32_t *__restrict__ heads, const int32_t *__restrict__ node_ids,
                                                        const int32_t *__restrict__ order, const int32_t *__restrict__ list, int64_t m,
                                                        int64_t branches, int32_t *__restrict__ brow, int32_t *__restrict__ branch /* nullable */,
                                                        int32_t *__restrict__ ids) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kCbBlock + threadIdx.x;
  if (s < branches) ids[s] = node_ids[heads[s]];
  if (s >= m) return;
  const int32_t b = node_branch[node_row[s]];
  brow[s] = b;
  if (branch) branch[list[order[s]]] = b >= 0 ? node_ids[heads[b]] : b;
}

// CB5's point words and CB6's moments, one lane per place.  A place of a junction or of a pruned node (row < 0) walks
// nothing and adds nothing.  table: rows of cb::kRowWords words with the host's graph words and the neutral elements of the
// minima in place; moments: rows of cd::kRowWords words, zeroed.
__global__ __launch_bounds__(kCbBlock) void k_cb_branches(const float *__restrict__ gx, const float *__restrict__ gy,
                                                          const float *__restrict__ gz, const int32_t *__restrict__ order, int64_t m,
                                                          GridDesc g, const int32_t *__restrict__ start, float t,
                                                          const int32_t *__restrict__ brow, const unsigned long long *__restrict__ dist,
                                                          const int32_t *__restrict__ list, int64_t n, const uint32_t *__restrict__ u32,
                                                          const unsigned long long *__restrict__ u64, unsigned long long *__restrict__ table,
                                                          unsigned long long *__restrict__ moments, uint32_t *__restrict__ words) {
  const int64_t s64 = static_cast<int64_t>(blockIdx.x) * kCbBlock + threadIdx.x;
  int32_t row = -1;
  if (s64 < m) row = brow[s64];
  const bool valid = row >= 0;
  gn::Moments mo;
  gn::clear(mo);
  unsigned long long points = 0, sum_w = 0, sx = 0, sy = 0, sz = 0, pos_min = ~0ull, pos_max = 0;
  uint32_t min_w = 0xffffffffu, max_w = 0;
  if (valid) {
    const int32_t s = static_cast<int32_t>(s64);
    const float qx = gx[s], qy = gy[s], qz = gz[s];
    // CB6: the ordered links of CC2 (gn::visit makes the test on d = fl32(p_j - p_i)) whose other end is of the same branch
    crack_walk<false>(g, start, qx, qy, qz, s, m, [&](int32_t c) {
      if (brow[c] == row) gn::visit(mo, gx[c] - qx, gy[c] - qy, gz[c] - qz, t);
    });
    if (mo.n >= gn::kMaxNeighbours) atomicMax(words + CB_OVER, 1u);
    const int32_t i = list[order[s]];
    const uint32_t w = cf::fused_w(u64[i], u32[n + i]);
    points = 1;
    sum_w = w;
    min_w = max_w = w;
    pos_min = pos_max = dist[s];
    sx = static_cast<unsigned long long>(cs::quant(qx));
    sy = static_cast<unsigned long long>(cs::quant(qy));
    sz = static_cast<unsigned long long>(cs::quant(qz));
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
    pos_min = wave_min_u64(pos_min);
    pos_max = wave_max_u64(pos_max);
  }
  if (issue) {
    unsigned long long *st = table + static_cast<int64_t>(cb::kRowWords) * row;
    atomicAdd(st + 6, points);
    atomicAdd(st + 7, sum_w);
    atomicMin(st + 8, static_cast<unsigned long long>(min_w));
    atomicMax(st + 9, static_cast<unsigned long long>(max_w));
    atomicMin(st + 10, pos_min);
    atomicMax(st + 11, pos_max);
    atomicAdd(st + 12, sx);
    atomicAdd(st + 13, sy);
    atomicAdd(st + 14, sz);
  }
  // CB6 (a lane that is not valid holds zeros)
  int64_t w[gn::kMomentWords];
  gn::store(mo, w);
  unsigned long long *out = moments + static_cast<int64_t>(cd::kRowWords) * (issue ? row : 0);
#pragma unroll
  for (int a = 0; a < gn::kMomentWords; ++a) {
    unsigned long long lo = cd::lo_of(w[a]), hi = static_cast<unsigned long long>(cd::hi_of(w[a]));
    if (shared) {
      lo = wave_sum_u64(lo);
      hi = wave_sum_u64(hi);
    }
    if (issue) {
      atomicAdd(out + 2 * a, lo);
      atomicAdd(out + 2 * a + 1, hi);
    }
  }
}

hipError_t preload_crack_branch() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_cb_branches));
}

// the m > 0 crack points, the nodes and the ordered edges the skeleton stage left in cc, cl, cs, cm.cs_* and ctx->g_*
int crack_branches_run(pcp_context *ctx, const pcp_crack_link_params &p, uint64_t step_q, uint64_t prune_q, const CcScratch &cc,
                       const ClScratch &cl, const CsScratch &cs, CbScratch &s, CrackCounts *c) {
  CrackMap &cm = *ctx->crack;
  const int64_t m = c->points, rows = c->cracks, nodes = c->nodes, edges = c->edges;
  const size_t sm = static_cast<size_t>(m), sk = static_cast<size_t>(nodes), sr = static_cast<size_t>(rows);
  const size_t pm = (sm + 3) & ~size_t(3);
  const float *gx = ctx->g_xyz.p, *gy = ctx->g_xyz.p + pm, *gz = ctx->g_xyz.p + 2 * pm;
  PCP_HIP_TRY(ctx, s.gather.ensure(2 * (sk + sr) + 4));
  PCP_HIP_TRY(ctx, s.words.ensure(CB_WORDS));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.words.p, 0, CB_WORDS * 4, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cb_gather, dim3(cb_blocks(std::max(nodes, rows))), dim3(kCbBlock), 0, ctx->stream, cm.cs_nodes.p, nodes, cl.end_a.p,
                       cl.end_b.p, cl.place_of.p, cs.node_row.p, rows, m, s.gather.p, s.words.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  std::vector<long long> gathered;
  std::vector<int64_t> node_crack, node_points;
  std::vector<int32_t> ends, up;
  cb::Graph g;
  uint32_t words[CB_WORDS] = {0, 0, 0, 0};
  try {
    gathered.resize(2 * (sk + sr));
    const hipError_t e1 = hipMemcpyAsync(gathered.data(), s.gather.p, gathered.size() * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipMemcpyAsync(words, s.words.p, sizeof(words), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e3 = hipStreamSynchronize(ctx->stream);  // (before any return: the copies write into this function's locals)
    PCP_HIP_TRY(ctx, e1);
    PCP_HIP_TRY(ctx, e2);
    PCP_HIP_TRY(ctx, e3);
    if (words[CB_BAD]) return set_error(ctx, PCP_ERR_DEVICE, "pcp_crack_branches: an end of a crack lies in no node");
    node_crack.resize(sk), node_points.resize(sk), ends.resize(2 * sr);
    for (size_t v = 0; v < sk; ++v) {
      node_crack[v] = gathered[2 * v], node_points[v] = gathered[2 * v + 1];
      if (node_crack[v] < 0 || node_crack[v] >= rows)
        return set_error(ctx, PCP_ERR_DEVICE, "pcp_crack_branches: node %lld is of crack row %lld of %lld", (long long)v, (long long)node_crack[v], (long long)rows);
    }
    for (size_t r = 0; r < 2 * sr; ++r) ends[r] = static_cast<int32_t>(gathered[2 * sk + r]);
    // CB2, CB3 and the graph words of CB5 and CB7
    cb::graph(nodes, node_crack.data(), node_points.data(), cm.cs_edges.data(), edges, rows, ends.data(), step_q, prune_q, g);
    up = g.node_branch;
    up.insert(up.end(), g.heads.begin(), g.heads.end());
    for (size_t b = 0; b < g.heads.size(); ++b) g.rows[cb::kRowWords * b + 8] = g.rows[cb::kRowWords * b + 10] = -1;  // (the minima: 2^64 - 1)
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_crack_branches: out of host memory for %lld nodes and %lld edges", (long long)nodes, (long long)edges);
  }
  const int64_t branches = static_cast<int64_t>(g.heads.size());
  const size_t sb = static_cast<size_t>(branches);
  PCP_HIP_TRY(ctx, s.node_branch.ensure(sk + sb + 4));
  PCP_HIP_TRY(ctx, s.brow.ensure(sm + 4));
  PCP_HIP_TRY(ctx, cm.cb_ids.ensure(sb + 4));
  PCP_HIP_TRY(ctx, cm.cb_table.ensure(static_cast<size_t>(cb::kRowWords) * sb + 4));
  PCP_HIP_TRY(ctx, cm.cb_moments.ensure(static_cast<size_t>(cd::kRowWords) * sb + 4));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(s.node_branch.p, up.data(), (sk + sb) * 4, hipMemcpyHostToDevice, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(cm.cb_table.p, g.rows.data(), static_cast<size_t>(cb::kRowWords) * sb * 8, hipMemcpyHostToDevice, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(cm.cb_moments.p, 0, static_cast<size_t>(cd::kRowWords) * sb * 8, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the uploads have read g and up)
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cb_assign, dim3(cb_blocks(m)), dim3(kCbBlock), 0, ctx->stream, cs.node_row.p, s.node_branch.p, s.node_branch.p + sk,
                       cm.cs_ids.p, ctx->g_order.p, cc.list.p, m, branches, s.brow.p, s.branch.p, cm.cb_ids.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cb_branches, dim3(cb_blocks(m)), dim3(kCbBlock), 0, ctx->stream, gx, gy, gz, ctx->g_order.p, m, cc.grid, ctx->g_start.p,
                       gn::threshold_of(p.radius), s.brow.p, cl.dist.p, cc.list.p, ctx->n, cm.cf_u32.p, cm.cf_u64.p, cm.cb_table.p, cm.cb_moments.p,
                       s.words.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  PCP_HIP_TRY(ctx, hipMemcpyAsync(words, s.words.p, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (words[CB_OVER])
    return set_error(ctx, PCP_ERR_RANGE, "pcp_crack_branches: a crack point has %lld links or more", static_cast<long long>(gn::kMaxNeighbours));
  cm.cb_edge_branch.swap(g.edge_branch);
  cm.cb_cracks.swap(g.cracks);
  c->branches = branches;
  c->pruned_branches = g.pruned_branches;
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

// CB1's checks after crack_link_check's, under the caller's name; the context's error where there is one
static int cb_check(pcp_context *ctx, const char *who, float radius, float step, float prune) {
  const float t = gn::threshold_of(radius);
  if (!cs::step_ok(step, t)) {
    const double least = static_cast<double>(cs::w_max_of(t)) * cl::kMetresPerUnit;
    if (ctx) return set_error(ctx, PCP_ERR_INVALID, "%s: step %g outside [%g, 16] (the longest link of radius %g)", who, static_cast<double>(step), least, static_cast<double>(radius));
    set_global_error("%s: step %g outside [%g, 16] (the longest link of radius %g)", who, static_cast<double>(step), least, static_cast<double>(radius));
    return PCP_ERR_INVALID;
  }
  if (!cb::prune_ok(prune)) {
    if (ctx) return set_error(ctx, PCP_ERR_INVALID, "%s: prune %g outside [0, 1024]", who, static_cast<double>(prune));
    set_global_error("%s: prune %g outside [0, 1024]", who, static_cast<double>(prune));
    return PCP_ERR_INVALID;
  }
  return PCP_OK;
}

extern "C" {

int pcp_crack_branches(pcp_context *ctx, const pcp_crack_link_params *p, float step, float prune, int32_t *out_branch, int64_t *out_branches,
                       int64_t *out_pruned_branches) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_branches) *out_branches = 0;
  if (out_pruned_branches) *out_pruned_branches = 0;
  int rc = crack_link_check(ctx, "pcp_crack_branches", p);
  if (rc != PCP_OK) return rc;
  if ((rc = cb_check(ctx, "pcp_crack_branches", p->radius, step, prune)) != PCP_OK) return rc;
  CrackOut out;
  out.branch = out_branch;
  CrackCounts c;
  if ((rc = crack_map_run(ctx, *p, CrackMap::kBranches, cs::step_q_of(step), out, &c, cb::prune_q_of(prune))) != PCP_OK) return rc;
  if (out_branches) *out_branches = c.branches;
  if (out_pruned_branches) *out_pruned_branches = c.pruned_branches;
  return PCP_OK;
}

int pcp_crack_branches_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows15, int64_t *out_moments20,
                             int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  const CrackMap &cm = *ctx->crack;
  int64_t rows = 0;
  const int rc = crack_window(ctx, "pcp_crack_branches_fetch", CrackMap::kBranches, first, max_rows, cm.cb_rows, &rows);
  if (rc != PCP_OK || rows == 0) return rc;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sr = static_cast<size_t>(rows), sf = static_cast<size_t>(first);
  if (out_id) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_id, cm.cb_ids.p + sf, sr * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_rows15)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rows15, cm.cb_table.p + cb::kRowWords * sf, cb::kRowWords * sr * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out_moments20)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_moments20, cm.cb_moments.p + cd::kRowWords * sf, cd::kRowWords * sr * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_crack_branch_edges_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_edge_branch, int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  const CrackMap &cm = *ctx->crack;
  int64_t rows = 0;
  const int rc = crack_window(ctx, "pcp_crack_branch_edges_fetch", CrackMap::kBranches, first, max_rows, static_cast<int64_t>(cm.cb_edge_branch.size()), &rows);
  if (rc != PCP_OK || rows == 0) return rc;
  if (out_edge_branch) std::copy(cm.cb_edge_branch.begin() + first, cm.cb_edge_branch.begin() + (first + rows), out_edge_branch);
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_crack_branch_cracks_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int64_t *out_rows7, int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  const CrackMap &cm = *ctx->crack;
  int64_t rows = 0;
  const int rc = crack_window(ctx, "pcp_crack_branch_cracks_fetch", CrackMap::kBranches, first, max_rows, static_cast<int64_t>(cm.cb_cracks.size() / cb::kCrackWords), &rows);
  if (rc != PCP_OK || rows == 0) return rc;
  if (out_rows7) std::copy(cm.cb_cracks.begin() + cb::kCrackWords * first, cm.cb_cracks.begin() + cb::kCrackWords * (first + rows), out_rows7);
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_crack_branch_lengths_host(int64_t nodes, const int64_t *rows10, int64_t edges, const int64_t *rows3, const int32_t *edge_branch,
                                  int64_t branches, int64_t cracks, double *out_length_m, double *out_kept_length_m) {
  if (nodes < 0 || edges < 0 || branches < 0 || cracks < 0 || (nodes > 0 && !rows10) || (edges > 0 && (!rows3 || !edge_branch)) ||
      (branches > 0 && !out_length_m) || (cracks > 0 && !out_kept_length_m)) {
    set_global_error("pcp_crack_branch_lengths_host: a negative count or a missing array");
    return PCP_ERR_INVALID;
  }
  for (int64_t v = 0; v < nodes; ++v)
    if (rows10[cs::kNodeWords * v] < 0 || rows10[cs::kNodeWords * v] >= cracks || rows10[cs::kNodeWords * v + 2] < 1) {
      set_global_error("pcp_crack_branch_lengths_host: node %lld is of crack row %lld of %lld or has no point", static_cast<long long>(v),
                       static_cast<long long>(rows10[cs::kNodeWords * v]), static_cast<long long>(cracks));
      return PCP_ERR_INVALID;
    }
  for (int64_t e = 0; e < edges; ++e)
    if (rows3[3 * e] < 0 || rows3[3 * e] >= nodes || rows3[3 * e + 1] < 0 || rows3[3 * e + 1] >= nodes || edge_branch[e] >= branches) {
      set_global_error("pcp_crack_branch_lengths_host: edge %lld names a node or a branch that is not there", static_cast<long long>(e));
      return PCP_ERR_INVALID;
    }
  cb::lengths(rows10, rows3, edge_branch, edges, branches, cracks, out_length_m, out_kept_length_m);
  return PCP_OK;
}

int pcp_crack_branches_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, float step, float prune,
                            const uint64_t *sum_q, int32_t *out_branch, int32_t *out_id, int64_t *out_rows15, int64_t *out_moments20,
                            int64_t edge_capacity, int32_t *out_edge_branch, int64_t *out_rows7, int64_t *out_branches, int64_t *out_edges,
                            int64_t *out_cracks) {
  if (out_branches) *out_branches = 0;
  if (out_edges) *out_edges = 0;
  if (out_cracks) *out_cracks = 0;
  if (!cf::min_views_ok(min_views) || !gn::radius_ok(radius)) {
    set_global_error("pcp_crack_branches_host: min_views %d outside %d..%d or radius %g outside [0.005, 1]", min_views, cf::kMinViewsLo,
                     cf::kMinViewsHi, static_cast<double>(radius));
    return PCP_ERR_INVALID;
  }
  if (cb_check(nullptr, "pcp_crack_branches_host", radius, step, prune) != PCP_OK) return PCP_ERR_INVALID;
  if (n < 0 || n > cf::kHostMaxPoints || edge_capacity < 0 || (n > 0 && (!xyz || !views))) {
    set_global_error("pcp_crack_branches_host: n outside 0..65536, a negative edge capacity or a missing array");
    return PCP_ERR_INVALID;
  }
  cb::HostResult res;
  cb::Brute how = cb::kBruteOk;
  try {
    how = cb::branches_brute(n, xyz, views, sum_q, min_views, gn::threshold_of(radius), cs::step_q_of(step), cb::prune_q_of(prune), res);
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_crack_branches_host: out of host memory for %lld points", static_cast<long long>(n));
    return PCP_ERR_NOMEM;
  }
  if (how == cb::kBruteRange || how == cb::kBruteLinks) {
    if (how == cb::kBruteRange)
      set_global_error("pcp_crack_branches_host: a crack point has a coordinate beyond 2^20 m");
    else
      set_global_error("pcp_crack_branches_host: a crack point has %lld links or more", static_cast<long long>(gn::kMaxNeighbours));
    return PCP_ERR_RANGE;
  }
  if (how != cb::kBruteOk) {
    set_global_error("pcp_crack_branches_host: a crack's diagram is not connected");
    return PCP_ERR_DEVICE;
  }
  const int64_t edges = static_cast<int64_t>(res.edge_branch.size());
  if (out_branch) std::copy(res.branch.begin(), res.branch.end(), out_branch);
  if (out_id) std::copy(res.ids.begin(), res.ids.end(), out_id);
  if (out_rows15) std::copy(res.rows.begin(), res.rows.end(), out_rows15);
  if (out_moments20) std::copy(res.moments.begin(), res.moments.end(), out_moments20);
  if (out_edge_branch) std::copy(res.edge_branch.begin(), res.edge_branch.begin() + std::min(edges, edge_capacity), out_edge_branch);
  if (out_rows7) std::copy(res.cracks.begin(), res.cracks.end(), out_rows7);
  if (out_branches) *out_branches = static_cast<int64_t>(res.ids.size());
  if (out_edges) *out_edges = edges;
  if (out_cracks) *out_cracks = static_cast<int64_t>(res.cracks.size() / cb::kCrackWords);
  return PCP_OK;
}

}  // extern "C"
