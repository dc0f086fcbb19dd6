// pcp_crack_fuse.hip -- crack widths on the map ("Crack widths on the map", CF1-CF6 and CC1-CC6): the widths
// pcp_crack_width measures per keyframe brought back to the map points that see them, and the map's cracks as connected
// components of the crack points -- what compute_skeleton_edge_pts of scripts/genNormAndDistanceMask.py (:396-478) leaves as
// one record per hand-picked pixel and crack_width_3d_results.json (:476-478) as a flat list without identity.
//
// Fusion: pcp_crack_fuse_add runs the keyframe's geometry scatter, distance transform and width kernels where
// pcp_crack_width runs them, keeps the flag and width images on the device, and a gather kernel, one lane per contributor of
// the keyframe (the list of pcp_frame_visible), folds the pixel's width into the point's own 40 B of state.  A point has one
// pixel per keyframe and a keyframe is added once, so the state needs no atomics; every field is an integer sum, count,
// minimum or maximum, so the final state does not depend on the order of the adds.
// Cracks: the crack points are compacted, binned into the uniform grid of the radius stages, and united by a lock-free
// union-find whose roots are the lowest indices (one lane per point over the 27 neighbouring cells, each pair once); a
// flatten pass writes the canonical labels, a scan ranks the roots, and a statistics kernel fills one row per crack with
// integer atomics, merged per wavefront where its lanes share a crack.
#include <algorithm>
#include <new>
#include <vector>

#include "pcp_device.hpp"
#include "pcp_crack_map.hpp"
#include "pcp_scan.hpp"
#include "pcp_crack_length.hpp"

namespace pcp {

constexpr int kCfBlock = 256;
constexpr int kCfU32Planes = 6;  // seen views centres min_q max_q best_q
constexpr int kCfU64Planes = 2;  // sum_q best_key

static inline uint32_t cf_blocks(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kCfBlock))); }

// ---- fusion ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCfBlock) void k_cf_init(uint32_t *__restrict__ u32, unsigned long long *__restrict__ u64, int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  if (i >= n) return;
  cf::State s;
  cf::clear(s);
  u32[i] = s.seen;
  u32[n + i] = s.views;
  u32[2 * n + i] = s.centres;
  u32[3 * n + i] = s.min_q;
  u32[4 * n + i] = s.max_q;
  u32[5 * n + i] = s.best_q;
  u64[i] = s.sum_q;
  u64[n + i] = s.best_key;
}

// CF1-CF4: one lane per contributor (entry k of the keyframe's list; the entries are distinct points, so no two lanes share
// a state).  tally[0] += credited contributors, one atomic per wavefront.
__global__ __launch_bounds__(kCfBlock) void k_cf_gather(const float *__restrict__ x, const float *__restrict__ y,
                                                        const float *__restrict__ z, DevCamera cam, DevFrame fr,
                                                        const int32_t *__restrict__ index, int64_t m, int64_t px,
                                                        const uint8_t *__restrict__ flags, const float *__restrict__ width,
                                                        int32_t frame, int64_t n, uint32_t *__restrict__ u32,
                                                        unsigned long long *__restrict__ u64, unsigned long long *__restrict__ tally) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  bool credited = false;
  if (k < m) {
    const int32_t i = index[k];
    const bool listed = i >= 0 && i < n;
    const Projected p = project_point(cam, fr.w2c, x[listed ? i : 0], y[listed ? i : 0], z[listed ? i : 0]);
    if (listed && p.pixel >= 0 && p.pixel < px) {  // (every entry of the list has a colour pixel; the tests stay as bounds)
      const float range = static_cast<float>(range64(p.xc, p.yc, p.zc));  // what k_gm_scatter keys the pixel's winner with
      const uint8_t f = flags[p.pixel];
      const float wv = (f & cf::kWidthFlag) ? width[p.pixel] : 0.0f;
      cf::State s;
      s.seen = u32[i];
      s.views = u32[n + i];
      s.centres = u32[2 * n + i];
      s.min_q = u32[3 * n + i];
      s.max_q = u32[4 * n + i];
      s.best_q = u32[5 * n + i];
      s.sum_q = u64[i];
      s.best_key = u64[n + i];
      credited = cf::update(s, f, wv, __float_as_uint(range), frame);
      u32[i] = s.seen;
      if (credited) {
        u32[n + i] = s.views;
        u32[2 * n + i] = s.centres;
        u32[3 * n + i] = s.min_q;
        u32[4 * n + i] = s.max_q;
        u32[5 * n + i] = s.best_q;
        u64[i] = s.sum_q;
        u64[n + i] = s.best_key;
      }
    }
  }
  const unsigned long long votes = __ballot(credited);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(tally, static_cast<unsigned long long>(__popcll(votes)));
}

// ---- cracks ---------------------------------------------------------------------------------------------------------------
// CC1
__global__ __launch_bounds__(kCfBlock) void k_cc_flag(const uint32_t *__restrict__ views, const float *__restrict__ x,
                                                      const float *__restrict__ y, const float *__restrict__ z, int64_t n,
                                                      int32_t min_views, uint8_t *__restrict__ flag) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  if (i >= n) return;
  flag[i] = cf::crack_point(views[i], min_views, x[i], y[i], z[i]) ? 1 : 0;
}

// the crack points as a view (point k of the view = input point list[k], ascending) and their box as ordered integers:
// box[0..2] = min, box[3..5] = max, one atomic of each per wavefront
__global__ __launch_bounds__(kCfBlock) void k_cc_gather(const int32_t *__restrict__ list, int64_t m, const float *__restrict__ x,
                                                        const float *__restrict__ y, const float *__restrict__ z,
                                                        float *__restrict__ vx, float *__restrict__ vy, float *__restrict__ vz,
                                                        uint32_t *__restrict__ box) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  cf::Box b;
  cf::clear(b);
  if (k < m) {
    const int32_t i = list[k];
    const float px = x[i], py = y[i], pz = z[i];
    vx[k] = px;
    vy[k] = py;
    vz[k] = pz;
    cf::add(b, px, py, pz);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const uint32_t lo = wave_min_u32(b.lo[a]), hi = wave_max_u32(b.hi[a]);
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
      atomicMin(box + a, lo);
      atomicMax(box + 3 + a, hi);
    }
  }
}

__global__ __launch_bounds__(kCfBlock) void k_cc_parent_init(int32_t *__restrict__ parent, int64_t m) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  if (k < m) parent[k] = static_cast<int32_t>(k);
}

// CC2: one lane per place s of the cell order; the candidates are the places after s in the rows of the neighbouring cells, so
// that every pair is tested once (the test is symmetric).  order[s] = the view index of place s.
__global__ __launch_bounds__(kCfBlock) void k_cc_union(const float *__restrict__ gx, const float *__restrict__ gy,
                                                       const float *__restrict__ gz, const int32_t *__restrict__ order, int64_t m,
                                                       GridDesc g, const int32_t *__restrict__ start, float t,
                                                       int32_t *__restrict__ parent) {
  const int64_t s64 = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  if (s64 >= m) return;
  const int32_t s = static_cast<int32_t>(s64);
  const float qx = gx[s], qy = gy[s], qz = gz[s];
  const int32_t mine = order[s];
  crack_walk<true>(g, start, qx, qy, qz, s, m, [&](int32_t c) {
    if (cl::d2_of(gx[c] - qx, gy[c] - qy, gz[c] - qz) <= t) cc_unite(parent, mine, order[c]);
  });
}

// CC3 (and CS3, without labels): after the union kernel has ended the forest is final; the walk goes down strictly descending
// indices.  label nullable.
__global__ __launch_bounds__(kCfBlock) void k_cc_flatten(const int32_t *__restrict__ parent, const int32_t *__restrict__ list,
                                                         int64_t m, int32_t *__restrict__ root_of, int32_t *__restrict__ is_root,
                                                         int32_t *__restrict__ label) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  if (k >= m) return;
  int32_t v = static_cast<int32_t>(k);
  for (int32_t p = parent[v]; p != v; p = parent[v]) v = p;  // (p < v)
  root_of[k] = v;
  is_root[k] = v == static_cast<int32_t>(k) ? 1 : 0;
  if (label) label[list[k]] = list[v];
}

// CC4: the empty table, and the ids (rank[k] = roots before view index k: the rows ascend by id because the list does)
__global__ __launch_bounds__(kCfBlock) void k_cc_table_init(unsigned long long *__restrict__ stats, uint32_t *__restrict__ box,
                                                            int64_t rows) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  if (r >= rows) return;
  stats[kCcStatWords * r + 0] = 0;
  stats[kCcStatWords * r + 1] = 0;
  stats[kCcStatWords * r + 2] = ~0ull;
  stats[kCcStatWords * r + 3] = 0;
  stats[kCcStatWords * r + 4] = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    box[6 * r + a] = 0xffffffffu;
    box[6 * r + 3 + a] = 0;
  }
}

__global__ __launch_bounds__(kCfBlock) void k_cc_ids(const int32_t *__restrict__ root_of, const int32_t *__restrict__ rank,
                                                     const int32_t *__restrict__ list, int64_t m, int32_t *__restrict__ ids) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  if (k >= m) return;
  if (root_of[k] == static_cast<int32_t>(k)) ids[rank[k]] = list[k];
}

// one lane per place of the cell order (neighbours in space are neighbours in the wavefront, and mostly of one crack): where
// all the lanes of a wavefront share a crack their values are merged first and one lane issues the atomics
__global__ __launch_bounds__(kCfBlock) void k_cc_stats(const float *__restrict__ gx, const float *__restrict__ gy,
                                                       const float *__restrict__ gz, const int32_t *__restrict__ order, int64_t m,
                                                       const int32_t *__restrict__ root_of, const int32_t *__restrict__ rank,
                                                       const int32_t *__restrict__ list, int64_t n, const uint32_t *__restrict__ u32,
                                                       const unsigned long long *__restrict__ u64,
                                                       unsigned long long *__restrict__ stats, uint32_t *__restrict__ box) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kCfBlock + threadIdx.x;
  const bool valid = s < m;
  int32_t row = -1;
  unsigned long long points = 0, sum_w = 0, centre = 0;
  uint32_t min_w = 0xffffffffu, max_w = 0;
  cf::Box b;
  cf::clear(b);
  if (valid) {
    const int32_t k = order[s];
    row = rank[root_of[k]];
    const int32_t i = list[k];
    const uint32_t w = cf::fused_w(u64[i], u32[n + i]);
    points = 1;
    sum_w = w;
    min_w = max_w = w;
    centre = u32[2 * n + i] > 0 ? 1 : 0;
    cf::add(b, gx[s], gy[s], gz[s]);
  }
  bool shared;
  const bool issue = wave_row_issuer(valid, row, &shared);
  if (shared) {
    points = wave_sum_u64(points);
    sum_w = wave_sum_u64(sum_w);
    centre = wave_sum_u64(centre);
    min_w = wave_min_u32(min_w);
    max_w = wave_max_u32(max_w);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      b.lo[a] = wave_min_u32(b.lo[a]);
      b.hi[a] = wave_max_u32(b.hi[a]);
    }
  }
  if (!issue) return;
  unsigned long long *st = stats + static_cast<int64_t>(kCcStatWords) * row;
  atomicAdd(st + 0, points);
  atomicAdd(st + 1, sum_w);
  atomicMin(st + 2, static_cast<unsigned long long>(min_w));
  atomicMax(st + 3, static_cast<unsigned long long>(max_w));
  if (centre) atomicAdd(st + 4, centre);
  uint32_t *bx = box + static_cast<int64_t>(6) * row;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMin(bx + a, b.lo[a]);
    atomicMax(bx + 3 + a, b.hi[a]);
  }
}

hipError_t preload_crack_fuse() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_cc_stats));
}

int crack_label_forest(pcp_context *ctx, const char *who, const char *what, const int32_t *parent, const int32_t *list, int64_t m,
                       int64_t least, int32_t *root_of, int32_t *rank, int32_t *label, int64_t *roots) {
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cc_flatten, dim3(cf_blocks(m)), dim3(kCfBlock), 0, ctx->stream, parent, list, m, root_of, rank, label);
    PCP_HIP_TRY(ctx, scan_exclusive(ctx->stream, rank, m + 1, ctx->s_tiles, nullptr));  // [m] = the number of roots
  }
  int32_t found = 0;
  PCP_HIP_TRY(ctx, hipMemcpyAsync(&found, rank + m, 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *roots = found;
  if (found < least || found > m)
    return set_error(ctx, PCP_ERR_DEVICE, "%s: %d %s for %lld crack points, outside %lld..%lld", who, found, what, (long long)m, (long long)least, (long long)m);
  return PCP_OK;
}

// the m > 0 crack points of s.list: view, grid, union, flatten, ranks, table
static int components_run(pcp_context *ctx, float radius, int64_t m, CcScratch &s, int64_t *out_components) {
  const int64_t n = ctx->n;
  CrackMap &cm = *ctx->crack;
  const size_t sm = static_cast<size_t>(m), pm = (sm + 3) & ~size_t(3);
  const size_t plane = (static_cast<size_t>(n) + 3) & ~size_t(3);
  const float *x = ctx->xyz.p, *y = ctx->xyz.p + plane, *z = ctx->xyz.p + 2 * plane;
  PCP_HIP_TRY(ctx, s.vxyz.ensure(3 * pm + 4));
  PCP_HIP_TRY(ctx, s.box.ensure(8));
  PCP_HIP_TRY(ctx, s.parent.ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.root_of.ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.rank.ensure(sm + 8));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.box.p, 0xff, 12, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.box.p + 3, 0, 12, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cc_gather, dim3(cf_blocks(m)), dim3(kCfBlock), 0, ctx->stream, s.list.p, m, x, y, z, s.vxyz.p, s.vxyz.p + pm,
                       s.vxyz.p + 2 * pm, s.box.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  uint32_t hbox[6] = {0, 0, 0, 0, 0, 0};
  PCP_HIP_TRY(ctx, hipMemcpyAsync(hbox, s.box.p, sizeof(hbox), hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  CloudView cv{};
  cv.x = s.vxyz.p;
  cv.y = s.vxyz.p + pm;
  cv.z = s.vxyz.p + 2 * pm;
  cv.n = m;
  cv.remap = nullptr;
  for (int a = 0; a < 3; ++a) {
    cv.mn[a] = cf::value_of(hbox[a]);
    cv.mx[a] = cf::value_of(hbox[3 + a]);
    s.lo[a] = cv.mn[a];
    s.hi[a] = cv.mx[a];
  }
  GridDesc g;
  int rc = build_radius_grid(ctx, cv, radius, &g);  // (ends the streams and the pcp_sor_partial that rest on the old grid)
  if (rc != PCP_OK) return rc;
  if (g.reach < 1 || g.reach > 2) return set_error(ctx, PCP_ERR_INVALID, "pcp_crack_components: grid reach %d outside 1..2", g.reach);
  const float *gx = ctx->g_xyz.p, *gy = ctx->g_xyz.p + pm, *gz = ctx->g_xyz.p + 2 * pm;
  s.grid = g;
  const float t = gn::threshold_of(radius);
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.rank.p, 0, (sm + 8) * 4, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cc_parent_init, dim3(cf_blocks(m)), dim3(kCfBlock), 0, ctx->stream, s.parent.p, m);
    hipLaunchKernelGGL(k_cc_union, dim3(cf_blocks(m)), dim3(kCfBlock), 0, ctx->stream, gx, gy, gz, ctx->g_order.p, m, g, ctx->g_start.p,
                       t, s.parent.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  int64_t rows = 0;
  if ((rc = crack_label_forest(ctx, "pcp_crack_components", "roots", s.parent.p, s.list.p, m, 1, s.root_of.p, s.rank.p, s.label.p, &rows)) != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, cm.cc_ids.ensure(static_cast<size_t>(rows) + 4));
  PCP_HIP_TRY(ctx, cm.cc_stats.ensure(static_cast<size_t>(kCcStatWords) * rows + 4));
  PCP_HIP_TRY(ctx, cm.cc_box.ensure(6 * static_cast<size_t>(rows) + 4));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cc_table_init, dim3(cf_blocks(rows)), dim3(kCfBlock), 0, ctx->stream, cm.cc_stats.p, cm.cc_box.p, rows);
    hipLaunchKernelGGL(k_cc_ids, dim3(cf_blocks(m)), dim3(kCfBlock), 0, ctx->stream, s.root_of.p, s.rank.p, s.list.p, m, cm.cc_ids.p);
    hipLaunchKernelGGL(k_cc_stats, dim3(cf_blocks(m)), dim3(kCfBlock), 0, ctx->stream, gx, gy, gz, ctx->g_order.p, m, s.root_of.p,
                       s.rank.p, s.list.p, n, cm.cf_u32.p, cm.cf_u64.p, cm.cc_stats.p, cm.cc_box.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  *out_components = rows;
  return PCP_OK;
}

int crack_link_check(pcp_context *ctx, const char *who, const pcp_crack_link_params *p) {
  if (!p) return set_error(ctx, PCP_ERR_INVALID, "%s: params is NULL", who);
  if (!cf::min_views_ok(p->min_views))
    return set_error(ctx, PCP_ERR_INVALID, "%s: min_views %d outside %d..%d", who, p->min_views, cf::kMinViewsLo, cf::kMinViewsHi);
  if (!gn::radius_ok(p->radius)) return set_error(ctx, PCP_ERR_INVALID, "%s: radius %g outside [0.005, 1]", who, static_cast<double>(p->radius));
  if (!ctx->crack->readable(CrackMap::kFusion)) return set_error(ctx, PCP_ERR_STATE, "%s: no accumulation (pcp_crack_fuse_begin)", who);
  return PCP_OK;
}

int crack_components_run(pcp_context *ctx, const pcp_crack_link_params &p, CcScratch &s, CrackCounts *c) {
  const int64_t n = ctx->n;
  const size_t sn = static_cast<size_t>(n);
  const size_t plane = (sn + 3) & ~size_t(3);
  PCP_HIP_TRY(ctx, s.flag.ensure(sn + 16));
  PCP_HIP_TRY(ctx, s.list.ensure(sn + 4));
  PCP_HIP_TRY(ctx, s.label.ensure(sn + 4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.label.p, 0xff, sn * 4, ctx->stream));  // CC3: -1 for a point that is no crack point
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cc_flag, dim3(cf_blocks(n)), dim3(kCfBlock), 0, ctx->stream, ctx->crack->cf_u32.p + sn, ctx->xyz.p, ctx->xyz.p + plane,
                       ctx->xyz.p + 2 * plane, n, p.min_views, s.flag.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  int rc = compact_flags(ctx, s.flag.p, n, s.list.p, n, &c->points);
  if (rc == PCP_OK && c->points > 0) rc = components_run(ctx, p.radius, c->points, s, &c->cracks);
  return rc;
}

// the stages up to `upto` and the copies of the per-point outputs, queued
static int crack_map_stages(pcp_context *ctx, const pcp_crack_link_params &p, CrackMap::Level upto, uint64_t step_q, const CrackOut &out,
                            CcScratch &cc, ClScratch &cl, CsScratch &cs, CbScratch &cb, uint64_t prune_q, CrackCounts *c) {
  const size_t sn = static_cast<size_t>(ctx->n);
  if (out.pos) {  // CL5: 2^64 - 1 for a point that is no crack point
    PCP_HIP_TRY(ctx, cl.pos.ensure(sn + 4));
    PCP_HIP_TRY(ctx, hipMemsetAsync(cl.pos.p, 0xff, sn * 8, ctx->stream));
  }
  if (out.node) {  // CS3: -1
    PCP_HIP_TRY(ctx, cs.node.ensure(sn + 4));
    PCP_HIP_TRY(ctx, hipMemsetAsync(cs.node.p, 0xff, sn * 4, ctx->stream));
  }
  if (out.branch) {  // CB4: -1
    PCP_HIP_TRY(ctx, cb.branch.ensure(sn + 4));
    PCP_HIP_TRY(ctx, hipMemsetAsync(cb.branch.p, 0xff, sn * 4, ctx->stream));
  }
  int rc = crack_components_run(ctx, p, cc, c);
  if (rc == PCP_OK && upto >= CrackMap::kLengths && c->points > 0) rc = crack_lengths_run(ctx, p, cc, cl, c);
  if (rc == PCP_OK && upto >= CrackMap::kSkeleton && c->points > 0) rc = crack_skeleton_run(ctx, p, step_q, cc, cl, cs, c);
  if (rc == PCP_OK && upto == CrackMap::kBranches && c->points > 0) rc = crack_branches_run(ctx, p, step_q, prune_q, cc, cl, cs, cb, c);
  if (rc != PCP_OK) return rc;
  if (out.label) PCP_HIP_TRY(ctx, hipMemcpyAsync(out.label, cc.label.p, sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out.pos) PCP_HIP_TRY(ctx, hipMemcpyAsync(out.pos, cl.pos.p, sn * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out.node) PCP_HIP_TRY(ctx, hipMemcpyAsync(out.node, cs.node.p, sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out.branch) PCP_HIP_TRY(ctx, hipMemcpyAsync(out.branch, cb.branch.p, sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  return PCP_OK;
}

int crack_map_run(pcp_context *ctx, const pcp_crack_link_params &p, CrackMap::Level upto, uint64_t step_q, const CrackOut &out,
                  CrackCounts *c, uint64_t prune_q) {
  CrackMap &cm = *ctx->crack;
  *c = CrackCounts();
  cm.replacing(upto);
  if (ctx->n == 0) {
    cm.hold(upto, *c);
    return PCP_OK;
  }
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  CcScratch cc;
  ClScratch cl;
  CsScratch cs;
  CbScratch cb;
  const int rc = crack_map_stages(ctx, p, upto, step_q, out, cc, cl, cs, cb, prune_q, c);
  const hipError_t e = hipStreamSynchronize(ctx->stream);  // (also: the scratch is released on return)
  drop_large_grid_bitmap(ctx);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, e);
  cm.hold(upto, *c);
  return PCP_OK;
}

int crack_window(pcp_context *ctx, const char *who, CrackMap::Level l, int64_t first, int64_t max_rows, int64_t have, int64_t *rows) {
  static const char *const maker[] = {"pcp_crack_fuse_begin", "pcp_crack_components", "pcp_crack_lengths", "pcp_crack_skeleton",
                                      "pcp_crack_directions", "pcp_crack_branches"};
  if (first < 0 || max_rows < 0) return set_error(ctx, PCP_ERR_INVALID, "%s: negative first or max_rows", who);
  if (!ctx->crack->readable(l)) return set_error(ctx, PCP_ERR_STATE, "%s: no table (%s on the accumulation as it is)", who, maker[l]);
  *rows = std::max<int64_t>(0, std::min(max_rows, have - first));
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_crack_fuse_begin(pcp_context *ctx) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!ctx->xyz.p && ctx->n > 0) return set_error(ctx, PCP_ERR_STATE, "pcp_crack_fuse_begin: no cloud uploaded");
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  CrackMap &cm = *ctx->crack;
  cm.release();
  const int64_t n = ctx->n;
  const size_t sn = static_cast<size_t>(n);
  PCP_HIP_TRY(ctx, cm.cf_u32.ensure(kCfU32Planes * sn + 4));
  PCP_HIP_TRY(ctx, cm.cf_u64.ensure(kCfU64Planes * sn + 4));
  try {
    cm.cf_added.assign(static_cast<size_t>(std::max<int32_t>(ctx->n_frames, 0)), 0);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_crack_fuse_begin: out of host memory for %d keyframes", ctx->n_frames);
  }
  if (n > 0) {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cf_init, dim3(cf_blocks(n)), dim3(kCfBlock), 0, ctx->stream, cm.cf_u32.p, cm.cf_u64.p, n);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  cm.begin();
  return PCP_OK;
}

int pcp_crack_fuse_add(pcp_context *ctx, int32_t frame, const pcp_crack_params *params, int64_t *out_contributors,
                       int64_t *out_credited) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_contributors) *out_contributors = 0;
  if (out_credited) *out_credited = 0;
  int rc = crack_width_check(ctx, "pcp_crack_fuse_add", params);
  if (rc != PCP_OK) return rc;
  CrackMap &cm = *ctx->crack;
  if (!cm.readable(CrackMap::kFusion)) return set_error(ctx, PCP_ERR_STATE, "pcp_crack_fuse_add: no accumulation (pcp_crack_fuse_begin on this cloud, camera and keyframes)");
  if (frame >= 0 && static_cast<size_t>(frame) < cm.cf_added.size() && cm.cf_added[static_cast<size_t>(frame)])
    return set_error(ctx, PCP_ERR_STATE, "pcp_crack_fuse_add: keyframe %d has been added to this accumulation", frame);
  // as pcp_crack_width: the geometry scatter (camera, cloud, keyframes, the keyframe's range), the distance transform (the mask),
  // the width kernels; the flag and width images stay in ctx->cw_flags and ctx->cw_f32
  int64_t m = 0;
  if ((rc = frame_geometry_device(ctx, "pcp_crack_fuse_add", frame, /*with_normals=*/false, &m)) != PCP_OK) return rc;
  const int64_t px = static_cast<int64_t>(ctx->dcam.img_w) * ctx->dcam.img_h;
  unsigned long long credited = 0;
  if (px > 0) {
    if ((rc = mask_edt_device(ctx, "pcp_crack_fuse_add", frame, params->threshold)) != PCP_OK) return rc;
    const CrackWidthWant want{true, false, false, true, false, false, false};
    if ((rc = crack_width_device(ctx, *params, want)) != PCP_OK) return rc;
    // CF1: the keyframe's list is still in ctx->s_cell -- neither the distance transform nor the width kernels compact
    // anything or touch the single-keyframe scratch
    unsigned long long *tally = ctx->s_counter.p + 1;  // (word 0: the scatter's occupied count; 2, 3: the width kernels' counts)
    PCP_HIP_TRY(ctx, hipMemsetAsync(tally, 0, 8, ctx->stream));
    if (m > 0) {
      const size_t plane = (static_cast<size_t>(ctx->n) + 3) & ~size_t(3);
      const size_t spx = static_cast<size_t>(px);
      LaunchTimer lt(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_cf_gather, dim3(cf_blocks(m)), dim3(kCfBlock), 0, ctx->stream, ctx->xyz.p, ctx->xyz.p + plane,
                         ctx->xyz.p + 2 * plane, ctx->dcam, ctx->hframes[static_cast<size_t>(frame)], ctx->s_cell.p, m, px,
                         ctx->cw_flags.p, ctx->cw_f32.p + 4 * spx, frame, ctx->n, cm.cf_u32.p, cm.cf_u64.p, tally);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    PCP_HIP_TRY(ctx, hipMemcpyAsync(&credited, tally, 8, hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  cm.cf_added[static_cast<size_t>(frame)] = 1;
  cm.changed();
  if (out_contributors) *out_contributors = m;
  if (out_credited) *out_credited = static_cast<int64_t>(credited);
  return PCP_OK;
}

int pcp_crack_fuse_fetch(pcp_context *ctx, float *out_width_mean, float *out_width_best, int32_t *out_best_frame, uint32_t *out_views,
                         uint32_t *out_seen, uint32_t *out_centres, uint32_t *out_min_q, uint32_t *out_max_q, uint64_t *out_sum_q) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!ctx->crack->readable(CrackMap::kFusion)) return set_error(ctx, PCP_ERR_STATE, "pcp_crack_fuse_fetch: no accumulation (pcp_crack_fuse_begin)");
  const int64_t n = ctx->n;
  if (n == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sn = static_cast<size_t>(n);
  // CF5 is taken on the host from the planes it reads; a plane the caller did not ask for goes through a vector of the call's own
  std::vector<uint32_t> own_views, own_best_q;
  std::vector<uint64_t> own_sum, own_key;
  const bool derived = out_width_mean || out_width_best || out_best_frame;
  try {
    if (derived && !out_views) own_views.resize(sn);
    if (out_width_mean && !out_sum_q) own_sum.resize(sn);
    if (out_width_best) own_best_q.resize(sn);
    if (out_best_frame) own_key.resize(sn);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_crack_fuse_fetch: out of host memory for %lld points", static_cast<long long>(n));
  }
  uint32_t *views = out_views ? out_views : (own_views.empty() ? nullptr : own_views.data());
  uint64_t *sum_q = out_sum_q ? out_sum_q : (own_sum.empty() ? nullptr : own_sum.data());
  const uint32_t *u32 = ctx->crack->cf_u32.p;
  const unsigned long long *u64 = ctx->crack->cf_u64.p;
  hipStream_t st = ctx->stream;
  if (out_seen) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_seen, u32, sn * 4, hipMemcpyDeviceToHost, st));
  if (views) PCP_HIP_TRY(ctx, hipMemcpyAsync(views, u32 + sn, sn * 4, hipMemcpyDeviceToHost, st));
  if (out_centres) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_centres, u32 + 2 * sn, sn * 4, hipMemcpyDeviceToHost, st));
  if (out_min_q) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_min_q, u32 + 3 * sn, sn * 4, hipMemcpyDeviceToHost, st));
  if (out_max_q) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_max_q, u32 + 4 * sn, sn * 4, hipMemcpyDeviceToHost, st));
  if (!own_best_q.empty()) PCP_HIP_TRY(ctx, hipMemcpyAsync(own_best_q.data(), u32 + 5 * sn, sn * 4, hipMemcpyDeviceToHost, st));
  if (sum_q) PCP_HIP_TRY(ctx, hipMemcpyAsync(sum_q, u64, sn * 8, hipMemcpyDeviceToHost, st));
  if (!own_key.empty()) PCP_HIP_TRY(ctx, hipMemcpyAsync(own_key.data(), u64 + sn, sn * 8, hipMemcpyDeviceToHost, st));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(st));
  for (size_t i = 0; i < sn && derived; ++i) {
    if (out_width_mean) out_width_mean[i] = cf::width_mean(sum_q[i], views[i]);
    if (out_width_best) out_width_best[i] = cf::width_best(own_best_q[i], views[i]);
    if (out_best_frame) out_best_frame[i] = cf::best_frame(own_key[i], views[i]);
  }
  return PCP_OK;
}

int pcp_crack_fuse_end(pcp_context *ctx) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!ctx->crack->readable(CrackMap::kFusion)) return set_error(ctx, PCP_ERR_STATE, "pcp_crack_fuse_end: no accumulation (pcp_crack_fuse_begin)");
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->crack->release();
  return PCP_OK;
}

int pcp_crack_fuse_host(int64_t n, uint32_t *seen, uint32_t *views, uint32_t *centres, uint32_t *min_q, uint32_t *max_q,
                        uint32_t *best_q, uint64_t *sum_q, uint64_t *best_key, int64_t m, const int32_t *index, const int32_t *pixel,
                        const float *range, int32_t frame, int32_t width, int32_t height, const uint8_t *flags, const float *width_image,
                        int64_t *out_credited) {
  if (out_credited) *out_credited = 0;
  if (n < 0 || m < 0 || frame < 0 || width < 0 || height < 0 ||
      (n > 0 && (!seen || !views || !centres || !min_q || !max_q || !best_q || !sum_q || !best_key)) ||
      (m > 0 && (!index || !pixel || !range || !flags || !width_image))) {
    set_global_error("pcp_crack_fuse_host: a negative size or keyframe, or a missing array");
    return PCP_ERR_INVALID;
  }
  const int64_t px = static_cast<int64_t>(width) * height;
  for (int64_t k = 0; k < m; ++k)  // nothing changes unless every entry is good
    if (index[k] < 0 || index[k] >= n || pixel[k] < 0 || pixel[k] >= px || !(range[k] > 0.0f) || !(range[k] <= 3.402823466e+38f)) {
      set_global_error("pcp_crack_fuse_host: contributor %lld: index %d outside 0..n-1, pixel %d outside the image, or a range that is not positive and finite",
                       static_cast<long long>(k), index[k], pixel[k]);
      return PCP_ERR_INVALID;
    }
  int64_t credited = 0;
  for (int64_t k = 0; k < m; ++k) {
    const int32_t i = index[k];
    cf::State s{seen[i], views[i], centres[i], min_q[i], max_q[i], best_q[i], sum_q[i], best_key[i]};
    uint32_t bits;
    std::memcpy(&bits, &range[k], 4);
    credited += cf::update(s, flags[pixel[k]], width_image[pixel[k]], bits, frame) ? 1 : 0;
    seen[i] = s.seen;
    views[i] = s.views;
    centres[i] = s.centres;
    min_q[i] = s.min_q;
    max_q[i] = s.max_q;
    best_q[i] = s.best_q;
    sum_q[i] = s.sum_q;
    best_key[i] = s.best_key;
  }
  if (out_credited) *out_credited = credited;
  return PCP_OK;
}

int pcp_crack_components(pcp_context *ctx, const pcp_crack_link_params *p, int32_t *out_label, int64_t *out_crack_points,
                         int64_t *out_components) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_crack_points) *out_crack_points = 0;
  if (out_components) *out_components = 0;
  int rc = crack_link_check(ctx, "pcp_crack_components", p);
  if (rc != PCP_OK) return rc;
  CrackOut out;
  out.label = out_label;
  CrackCounts c;
  if ((rc = crack_map_run(ctx, *p, CrackMap::kComponents, 0, out, &c)) != PCP_OK) return rc;
  if (out_crack_points) *out_crack_points = c.points;
  if (out_components) *out_components = c.cracks;
  return PCP_OK;
}

int pcp_crack_components_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_stats, float *out_box,
                               int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  const CrackMap &cm = *ctx->crack;
  int64_t rows = 0;
  const int rc = crack_window(ctx, "pcp_crack_components_fetch", CrackMap::kComponents, first, max_rows, cm.cc_rows, &rows);
  if (rc != PCP_OK || rows == 0) return rc;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sr = static_cast<size_t>(rows), sf = static_cast<size_t>(first);
  std::vector<uint32_t> box;
  try {
    if (out_box) box.resize(6 * sr);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_crack_components_fetch: out of host memory for %lld rows", static_cast<long long>(rows));
  }
  if (out_id) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_id, cm.cc_ids.p + sf, sr * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_stats)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_stats, cm.cc_stats.p + kCcStatWords * sf, kCcStatWords * sr * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out_box) PCP_HIP_TRY(ctx, hipMemcpyAsync(box.data(), cm.cc_box.p + 6 * sf, 6 * sr * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < box.size(); ++k) out_box[k] = cf::value_of(box[k]);
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_crack_components_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, int32_t *out_label,
                              int64_t *out_components) {
  if (out_components) *out_components = 0;
  if (!cf::min_views_ok(min_views) || !gn::radius_ok(radius)) {
    set_global_error("pcp_crack_components_host: min_views %d outside %d..%d or radius %g outside [0.005, 1]", min_views, cf::kMinViewsLo,
                     cf::kMinViewsHi, static_cast<double>(radius));
    return PCP_ERR_INVALID;
  }
  if (n < 0 || n > cf::kHostMaxPoints || (n > 0 && (!xyz || !views || !out_label))) {
    set_global_error("pcp_crack_components_host: n outside 0..65536 or a missing array");
    return PCP_ERR_INVALID;
  }
  int64_t components = 0;
  try {
    components = cf::label_brute(n, xyz, views, min_views, gn::threshold_of(radius), out_label);
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_crack_components_host: out of host memory for %lld points", static_cast<long long>(n));
    return PCP_ERR_NOMEM;
  }
  if (out_components) *out_components = components;
  return PCP_OK;
}

}  // extern "C"
