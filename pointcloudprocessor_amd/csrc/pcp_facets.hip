// pcp_facets.hip -- planar facets of the map ("Planar facets", FA1-FA9): the faces of the structure as connected
// components of the map points under a link of distance, normal angle and mutual plane distance, one row of exact integers
// per face -- what PCL users know as RegionGrowing / ConditionalEuclideanClustering, stated as the components of a symmetric
// integer predicate so that the result does not depend on the order of points, lanes and atomics.  The reference's scripts stop
// at per-keyframe pictures; nothing there partitions the map.
//
// The facet points are flagged and compacted, binned into the uniform grid of the radius stages and united by the crack
// chain's lock-free union-find (pcp_crack_map.hpp: cc_unite, roots are the lowest indices), one lane per place of the cell
// order over the neighbouring cells, each pair once; the candidate's 12 B of coordinates decide the fp32 distance test and
// only a candidate that passes it has its 8-byte normal record read.  The chain's flatten and rank pass gives the components;
// a count-and-box kernel, a scan over the components that reach min_points, and a second pass for the moments about each
// facet's root point fill the table, both merged per wavefront where the lanes share a row.  The arithmetic is
// pcp_facets.hpp's, shared with pcp_facets_host.
// Opt-in: nothing here runs unless one of its entry points is called.
#include <algorithm>
#include <new>
#include <vector>

#include "pcp_crack_map.hpp"
#include "pcp_crack_length.hpp"
#include "pcp_facets.hpp"
#include "pcp_scan.hpp"

namespace pcp {

constexpr int kFaBlock = 256;

static inline uint32_t fa_blocks(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kFaBlock))); }

// FA2: one lane per input point
__global__ __launch_bounds__(kFaBlock) void k_fa_flag(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                      const float4 *__restrict__ normals, int64_t n, float max_curvature,
                                                      uint8_t *__restrict__ flag) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kFaBlock + threadIdx.x;
  if (i >= n) return;
  const float4 nc = normals[i];
  flag[i] = fa::facet_point(x[i], y[i], z[i], nc.x, nc.y, nc.z, nc.w, max_curvature) ? 1 : 0;
}

// the facet points as a view (point k of the view = input point list[k], ascending), their box as ordered integers (box[0..2]
// = min, box[3..5] = max, one atomic of each per wavefront) and every point its own parent
__global__ __launch_bounds__(kFaBlock) void k_fa_view(const int32_t *__restrict__ list, int64_t m, const float *__restrict__ x,
                                                      const float *__restrict__ y, const float *__restrict__ z, float *__restrict__ vx,
                                                      float *__restrict__ vy, float *__restrict__ vz, uint32_t *__restrict__ box,
                                                      int32_t *__restrict__ parent) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kFaBlock + threadIdx.x;
  cf::Box b;
  cf::clear(b);
  if (k < m) {
    const int32_t i = list[k];
    const float px = x[i], py = y[i], pz = z[i];
    vx[k] = px;
    vy[k] = py;
    vz[k] = pz;
    parent[k] = static_cast<int32_t>(k);
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

// FA3: quantise and pack, gathered in cell order: rec[s] = the record of the point at place s
__global__ __launch_bounds__(kFaBlock) void k_fa_records(const int32_t *__restrict__ order, const int32_t *__restrict__ list, int64_t m,
                                                         const float4 *__restrict__ normals, uint2 *__restrict__ rec) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kFaBlock + threadIdx.x;
  if (s >= m) return;
  const float4 nc = normals[list[order[s]]];
  uint32_t lo, hi;
  fa::pack(fa::normal_of(nc.x, nc.y, nc.z), true, &lo, &hi);
  rec[s] = make_uint2(lo, hi);
}

// FA4 / FA8: one lane per place s of the cell order; the candidates are the places after s in the rows of the neighbouring
// cells, so that every pair is tested once (the link is symmetric).  No lane waits for another one (cc_unite).
__global__ __launch_bounds__(kFaBlock) void k_fa_union(const float *__restrict__ gx, const float *__restrict__ gy,
                                                       const float *__restrict__ gz, const uint2 *__restrict__ rec,
                                                       const int32_t *__restrict__ order, int64_t m, GridDesc g,
                                                       const int32_t *__restrict__ start, fa::Link l, int32_t *__restrict__ parent) {
  const int64_t s64 = static_cast<int64_t>(blockIdx.x) * kFaBlock + threadIdx.x;
  if (s64 >= m) return;
  const int32_t s = static_cast<int32_t>(s64);
  const float qx = gx[s], qy = gy[s], qz = gz[s];
  const uint2 own = rec[s];
  const fa::Normal ni = fa::unpack(own.x, own.y);
  const int32_t mine = order[s];
  crack_walk<true>(g, start, qx, qy, qz, s, m, [&](int32_t c) {
    const float dx = gx[c] - qx, dy = gy[c] - qy, dz = gz[c] - qz;
    if (!(cl::d2_of(dx, dy, dz) <= l.t)) return;
    const uint2 other = rec[c];
    if (fa::linked(dx, dy, dz, ni, fa::unpack(other.x, other.y), l)) cc_unite(parent, mine, order[c]);
  });
}

// FA6, first pass: one lane per place of the cell order (neighbours in space are neighbours in the wavefront, and mostly of
// one component): count and box per component, merged over the wavefront where all its lanes share the row
__global__ __launch_bounds__(kFaBlock) void k_fa_stats(const float *__restrict__ gx, const float *__restrict__ gy,
                                                       const float *__restrict__ gz, const int32_t *__restrict__ order, int64_t m,
                                                       const int32_t *__restrict__ root_of, const int32_t *__restrict__ rank,
                                                       unsigned long long *__restrict__ count, uint32_t *__restrict__ box) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kFaBlock + threadIdx.x;
  const bool valid = s < m;
  int32_t row = -1;
  unsigned long long points = 0;
  cf::Box b;
  cf::clear(b);
  if (valid) {
    row = rank[root_of[order[s]]];
    points = 1;
    cf::add(b, gx[s], gy[s], gz[s]);
  }
  bool shared;
  const bool issue = wave_row_issuer(valid, row, &shared);
  if (shared) {
    points = wave_sum_u64(points);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      b.lo[a] = wave_min_u32(b.lo[a]);
      b.hi[a] = wave_max_u32(b.hi[a]);
    }
  }
  if (!issue) return;
  atomicAdd(count + row, points);
  uint32_t *bx = box + static_cast<int64_t>(6) * row;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMin(bx + a, b.lo[a]);
    atomicMax(bx + 3 + a, b.hi[a]);
  }
}

__global__ __launch_bounds__(kFaBlock) void k_fa_stats_init(unsigned long long *__restrict__ count, uint32_t *__restrict__ box, int64_t rows) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kFaBlock + threadIdx.x;
  if (r >= rows) return;
  count[r] = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    box[6 * r + a] = 0xffffffffu;
    box[6 * r + 3 + a] = 0;
  }
}

// FA5: keep[r] = 1 for a component with min_points members or more (scanned into the facets' rows afterwards)
__global__ __launch_bounds__(kFaBlock) void k_fa_keep(const unsigned long long *__restrict__ count, int64_t rows, int32_t min_points,
                                                      int32_t *__restrict__ keep) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kFaBlock + threadIdx.x;
  if (r < rows) keep[r] = count[r] >= static_cast<unsigned long long>(min_points) ? 1 : 0;
}

// FA5: one lane per view index; frow = the exclusive scan of keep (rows + 1 entries), so component r is a facet iff
// frow[r + 1] != frow[r] and its row is frow[r].  Clears the labels of the points of the other components; the root of a
// facet writes the facet's id, count (with zeroed moments) and box.
__global__ __launch_bounds__(kFaBlock) void k_fa_small(const int32_t *__restrict__ root_of, const int32_t *__restrict__ rank,
                                                       const int32_t *__restrict__ frow, const int32_t *__restrict__ list, int64_t m,
                                                       const unsigned long long *__restrict__ count, const uint32_t *__restrict__ box,
                                                       int32_t *__restrict__ label, int32_t *__restrict__ ids, long long *__restrict__ table,
                                                       uint32_t *__restrict__ fbox) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kFaBlock + threadIdx.x;
  if (k >= m) return;
  const int32_t r = rank[root_of[k]];
  const int32_t f = frow[r];
  if (frow[r + 1] == f) {
    label[list[k]] = -1;
    return;
  }
  if (root_of[k] != static_cast<int32_t>(k)) return;
  ids[f] = list[k];
  long long *row = table + static_cast<int64_t>(fa::kRowWords) * f;
  row[0] = static_cast<long long>(count[r]);
#pragma unroll
  for (int a = 1; a < fa::kRowWords; ++a) row[a] = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) fbox[static_cast<int64_t>(6) * f + a] = box[static_cast<int64_t>(6) * r + a];
}

// FA6, second pass: one lane per place; the nine sums of Q = rint(fl32(p - p_root) * 2^12) per facet, merged over the
// wavefront where its lanes share the facet, then one atomic per word (two's complement: the sums are signed)
__global__ __launch_bounds__(kFaBlock) void k_fa_moments(const float *__restrict__ gx, const float *__restrict__ gy,
                                                         const float *__restrict__ gz, const int32_t *__restrict__ order, int64_t m,
                                                         const float *__restrict__ vx, const float *__restrict__ vy,
                                                         const float *__restrict__ vz, const int32_t *__restrict__ root_of,
                                                         const int32_t *__restrict__ rank, const int32_t *__restrict__ frow,
                                                         long long *__restrict__ table) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kFaBlock + threadIdx.x;
  bool valid = false;
  int32_t row = -1;
  int64_t w[fa::kRowWords];
#pragma unroll
  for (int a = 0; a < fa::kRowWords; ++a) w[a] = 0;
  if (s < m) {
    const int32_t root = root_of[order[s]];
    const int32_t r = rank[root];
    row = frow[r];
    valid = frow[r + 1] != row;
    if (valid) fa::add_member(w, fa::moment_q(gx[s] - vx[root]), fa::moment_q(gy[s] - vy[root]), fa::moment_q(gz[s] - vz[root]));
  }
  bool shared;
  const bool issue = wave_row_issuer(valid, row, &shared);
  if (shared) {
#pragma unroll
    for (int a = 1; a < fa::kRowWords; ++a) w[a] = static_cast<int64_t>(wave_sum_u64(static_cast<unsigned long long>(w[a])));
  }
  if (!issue) return;
  unsigned long long *out = reinterpret_cast<unsigned long long *>(table) + static_cast<int64_t>(fa::kRowWords) * row;
#pragma unroll
  for (int a = 1; a < fa::kRowWords; ++a)
    if (w[a]) atomicAdd(out + a, static_cast<unsigned long long>(w[a]));
}

hipError_t preload_facets() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_fa_union));
}

// per-call scratch, released when the call returns: sized by the facet points (m) and the components (rows)
struct FaScratch {
  DevBuf<uint8_t> flag;
  DevBuf<int32_t> list, parent, root_of, rank, frow;
  DevBuf<float> vxyz;
  DevBuf<uint32_t> gbox, cbox;
  DevBuf<uint2> rec;
  DevBuf<unsigned long long> count;
};

struct FaCounts {
  int64_t points = 0, components = 0, facets = 0;
};

// the m > 0 facet points of s.list: view, grid, records, union, components, the facets' table
static int facets_components(pcp_context *ctx, const pcp_facet_params &p, const fa::Link &l, int64_t m, FaScratch &s, FaCounts *c) {
  const int64_t n = ctx->n;
  Facets &fs = ctx->facets;
  const size_t sm = static_cast<size_t>(m), pm = (sm + 3) & ~size_t(3);
  const size_t plane = (static_cast<size_t>(n) + 3) & ~size_t(3);
  const float *x = ctx->xyz.p, *y = ctx->xyz.p + plane, *z = ctx->xyz.p + 2 * plane;
  const float4 *normals = reinterpret_cast<const float4 *>(ctx->gn_normal.p);
  PCP_HIP_TRY(ctx, s.vxyz.ensure(3 * pm + 4));
  PCP_HIP_TRY(ctx, s.gbox.ensure(8));
  PCP_HIP_TRY(ctx, s.parent.ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.root_of.ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.rank.ensure(sm + 8));
  PCP_HIP_TRY(ctx, s.rec.ensure(sm + 4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.gbox.p, 0xff, 12, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.gbox.p + 3, 0, 12, ctx->stream));
  float *vx = s.vxyz.p, *vy = s.vxyz.p + pm, *vz = s.vxyz.p + 2 * pm;
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_fa_view, dim3(fa_blocks(m)), dim3(kFaBlock), 0, ctx->stream, s.list.p, m, x, y, z, vx, vy, vz, s.gbox.p, s.parent.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  uint32_t hbox[6] = {0, 0, 0, 0, 0, 0};
  PCP_HIP_TRY(ctx, hipMemcpyAsync(hbox, s.gbox.p, sizeof(hbox), hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  CloudView cv{};
  cv.x = vx;
  cv.y = vy;
  cv.z = vz;
  cv.n = m;
  cv.remap = nullptr;
  for (int a = 0; a < 3; ++a) {
    cv.mn[a] = cf::value_of(hbox[a]);
    cv.mx[a] = cf::value_of(hbox[3 + a]);
  }
  GridDesc g;
  int rc = build_radius_grid(ctx, cv, p.link_radius, &g);  // FA9 (ends the streams and the pcp_sor_partial that rest on the old grid)
  if (rc != PCP_OK) return rc;
  if (g.reach < 1 || g.reach > 2) return set_error(ctx, PCP_ERR_INVALID, "pcp_facets: grid reach %d outside 1..2", g.reach);
  const float *gx = ctx->g_xyz.p, *gy = ctx->g_xyz.p + pm, *gz = ctx->g_xyz.p + 2 * pm;
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.rank.p, 0, (sm + 8) * 4, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_fa_records, dim3(fa_blocks(m)), dim3(kFaBlock), 0, ctx->stream, ctx->g_order.p, s.list.p, m, normals, s.rec.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_fa_union, dim3(fa_blocks(m)), dim3(kFaBlock), 0, ctx->stream, gx, gy, gz, s.rec.p, ctx->g_order.p, m, g, ctx->g_start.p, l,
                       s.parent.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  int64_t rows = 0;
  if ((rc = crack_label_forest(ctx, "pcp_facets", "roots", s.parent.p, s.list.p, m, 1, s.root_of.p, s.rank.p, fs.label.p, &rows)) != PCP_OK) return rc;
  c->components = rows;
  const size_t sr = static_cast<size_t>(rows);
  PCP_HIP_TRY(ctx, s.count.ensure(sr + 4));
  PCP_HIP_TRY(ctx, s.cbox.ensure(6 * sr + 4));
  PCP_HIP_TRY(ctx, s.frow.ensure(sr + 8));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.frow.p, 0, (sr + 8) * 4, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_fa_stats_init, dim3(fa_blocks(rows)), dim3(kFaBlock), 0, ctx->stream, s.count.p, s.cbox.p, rows);
    hipLaunchKernelGGL(k_fa_stats, dim3(fa_blocks(m)), dim3(kFaBlock), 0, ctx->stream, gx, gy, gz, ctx->g_order.p, m, s.root_of.p, s.rank.p,
                       s.count.p, s.cbox.p);
    hipLaunchKernelGGL(k_fa_keep, dim3(fa_blocks(rows)), dim3(kFaBlock), 0, ctx->stream, s.count.p, rows, p.min_points, s.frow.p);
    PCP_HIP_TRY(ctx, scan_exclusive(ctx->stream, s.frow.p, rows + 1, ctx->s_tiles, nullptr));  // [rows] = the number of facets
  }
  int32_t facets = 0;
  PCP_HIP_TRY(ctx, hipMemcpyAsync(&facets, s.frow.p + rows, 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (facets < 0 || facets > rows)
    return set_error(ctx, PCP_ERR_DEVICE, "pcp_facets: %d facets of %lld components", facets, static_cast<long long>(rows));
  c->facets = facets;
  const size_t sf = static_cast<size_t>(facets);
  PCP_HIP_TRY(ctx, fs.ids.ensure(sf + 4));
  PCP_HIP_TRY(ctx, fs.table.ensure(fa::kRowWords * sf + 4));
  PCP_HIP_TRY(ctx, fs.box.ensure(6 * sf + 4));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_fa_small, dim3(fa_blocks(m)), dim3(kFaBlock), 0, ctx->stream, s.root_of.p, s.rank.p, s.frow.p, s.list.p, m, s.count.p,
                       s.cbox.p, fs.label.p, fs.ids.p, fs.table.p, fs.box.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  if (facets == 0) return PCP_OK;
  // FA6: every facet's sums stay below 2^62, checked on the host from the first pass before the second one runs
  std::vector<int32_t> ids;
  std::vector<long long> table;
  std::vector<uint32_t> box;
  try {
    ids.resize(sf);
    table.resize(fa::kRowWords * sf);
    box.resize(6 * sf);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_facets: out of host memory for %d facets", facets);
  }
  PCP_HIP_TRY(ctx, hipMemcpyAsync(ids.data(), fs.ids.p, sf * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(table.data(), fs.table.p, fa::kRowWords * sf * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(box.data(), fs.box.p, 6 * sf * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t f = 0; f < sf; ++f)
    if (!fa::moments_fit(table[fa::kRowWords * f], &box[6 * f]))
      return set_error(ctx, PCP_ERR_RANGE, "pcp_facets: facet %d (%lld points): points * (extent * 4096 + 1)^2 reaches 2^62, its moments could overflow",
                       ids[f], table[fa::kRowWords * f]);
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_fa_moments, dim3(fa_blocks(m)), dim3(kFaBlock), 0, ctx->stream, gx, gy, gz, ctx->g_order.p, m, vx, vy, vz, s.root_of.p,
                       s.rank.p, s.frow.p, fs.table.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return PCP_OK;
}

static int facets_stages(pcp_context *ctx, const pcp_facet_params &p, const fa::Link &l, FaScratch &s, int32_t *out_label, FaCounts *c) {
  const int64_t n = ctx->n;
  const size_t sn = static_cast<size_t>(n);
  const size_t plane = (sn + 3) & ~size_t(3);
  Facets &fs = ctx->facets;
  PCP_HIP_TRY(ctx, s.flag.ensure(sn + 16));
  PCP_HIP_TRY(ctx, s.list.ensure(sn + 4));
  PCP_HIP_TRY(ctx, fs.label.ensure(sn + 4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(fs.label.p, 0xff, sn * 4, ctx->stream));  // FA5: -1 for a point that is no facet point
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_fa_flag, dim3(fa_blocks(n)), dim3(kFaBlock), 0, ctx->stream, ctx->xyz.p, ctx->xyz.p + plane, ctx->xyz.p + 2 * plane,
                       reinterpret_cast<const float4 *>(ctx->gn_normal.p), n, p.max_curvature, s.flag.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  int rc = compact_flags(ctx, s.flag.p, n, s.list.p, n, &c->points);
  if (rc == PCP_OK && c->points > 0) rc = facets_components(ctx, p, l, c->points, s, c);
  if (rc != PCP_OK) return rc;
  if (out_label) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_label, fs.label.p, sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  return PCP_OK;
}

static int facets_check(const pcp_facet_params *p, const char **why) {
  *why = p ? fa::refusal(p->link_radius, p->angle_deg, p->plane_tol, p->max_curvature, p->min_points) : "params is NULL";
  return *why ? PCP_ERR_INVALID : PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_facets(pcp_context *ctx, const pcp_facet_params *params, int32_t *out_label, int64_t *out_facet_points, int64_t *out_components,
               int64_t *out_facets) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_facet_points) *out_facet_points = 0;
  if (out_components) *out_components = 0;
  if (out_facets) *out_facets = 0;
  const char *why = nullptr;
  if (facets_check(params, &why) != PCP_OK) return set_error(ctx, PCP_ERR_INVALID, "pcp_facets: %s", why);
  if (!ctx->xyz.p && ctx->n > 0) return set_error(ctx, PCP_ERR_STATE, "pcp_facets: no cloud uploaded");
  if (!ctx->gn_live) return set_error(ctx, PCP_ERR_STATE, "pcp_facets: no normals (pcp_estimate_normals on this cloud)");
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  Facets &fs = ctx->facets;
  fs.release();
  FaCounts c;
  if (ctx->n > 0) {
    const fa::Link l = fa::link_of(params->link_radius, params->angle_deg, params->plane_tol);
    FaScratch s;
    const int rc = facets_stages(ctx, *params, l, s, out_label, &c);
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (also: the scratch is released on return)
    drop_large_grid_bitmap(ctx);
    if (rc != PCP_OK) {
      fs.release();
      return rc;
    }
    PCP_HIP_TRY(ctx, e);
  }
  fs.rows = c.facets;
  fs.live = true;
  if (out_facet_points) *out_facet_points = c.points;
  if (out_components) *out_components = c.components;
  if (out_facets) *out_facets = c.facets;
  return PCP_OK;
}

int pcp_facets_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows10, float *out_box,
                     int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  if (first < 0 || max_rows < 0) return set_error(ctx, PCP_ERR_INVALID, "pcp_facets_fetch: negative first or max_rows");
  const Facets &fs = ctx->facets;
  if (!fs.live) return set_error(ctx, PCP_ERR_STATE, "pcp_facets_fetch: no table (pcp_facets on this cloud and these normals)");
  const int64_t rows = std::max<int64_t>(0, std::min(max_rows, fs.rows - first));
  if (rows == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sr = static_cast<size_t>(rows), sf = static_cast<size_t>(first);
  std::vector<uint32_t> box;
  try {
    if (out_box) box.resize(6 * sr);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_facets_fetch: out of host memory for %lld rows", static_cast<long long>(rows));
  }
  if (out_id) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_id, fs.ids.p + sf, sr * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_rows10)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rows10, fs.table.p + fa::kRowWords * sf, fa::kRowWords * sr * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out_box) PCP_HIP_TRY(ctx, hipMemcpyAsync(box.data(), fs.box.p + 6 * sf, 6 * sr * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < box.size(); ++k) out_box[k] = cf::value_of(box[k]);
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_facets_host(int64_t n, const float *xyz, const float *normal, const float *curvature, const pcp_facet_params *params,
                    int32_t *out_label, int32_t *out_id, int64_t *out_rows10, float *out_box, int64_t *out_facets) {
  if (out_facets) *out_facets = 0;
  const char *why = nullptr;
  if (facets_check(params, &why) != PCP_OK) {
    set_global_error("pcp_facets_host: %s", why);
    return PCP_ERR_INVALID;
  }
  if (n < 0 || n > fa::kHostMaxPoints || (n > 0 && (!xyz || !normal || !curvature))) {
    set_global_error("pcp_facets_host: n outside 0..65536 or a missing array");
    return PCP_ERR_INVALID;
  }
  fa::Table t;
  std::vector<int32_t> label;
  bool fit = true;
  try {
    label.resize(static_cast<size_t>(n));
    fit = fa::partition_brute(n, xyz, normal, curvature, fa::link_of(params->link_radius, params->angle_deg, params->plane_tol),
                              params->max_curvature, params->min_points, label.data(), t);
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_facets_host: out of host memory for %lld points", static_cast<long long>(n));
    return PCP_ERR_NOMEM;
  }
  if (!fit) {
    set_global_error("pcp_facets_host: facet %d: points * (extent * 4096 + 1)^2 reaches 2^62, its moments could overflow", t.unfit);
    return PCP_ERR_RANGE;
  }
  for (int64_t i = 0; i < n && out_label; ++i) out_label[i] = label[static_cast<size_t>(i)];
  for (size_t f = 0; f < t.ids.size(); ++f) {
    if (out_id) out_id[f] = t.ids[f];
    for (int a = 0; a < fa::kRowWords && out_rows10; ++a) out_rows10[fa::kRowWords * f + a] = t.rows[fa::kRowWords * f + a];
    for (int a = 0; a < 6 && out_box; ++a) out_box[6 * f + a] = cf::value_of(t.box[6 * f + a]);
  }
  if (out_facets) *out_facets = static_cast<int64_t>(t.ids.size());
  return PCP_OK;
}

int pcp_facet_plane_host(const float root[3], const int64_t row10[10], double out_plane[7]) {
  if (!root || !row10 || !out_plane) {
    set_global_error("pcp_facet_plane_host: a NULL argument");
    return PCP_ERR_INVALID;
  }
  if (!fa::plane_of(root, row10, out_plane)) {
    set_global_error("pcp_facet_plane_host: %lld points, a facet has one at least", static_cast<long long>(row10[0]));
    return PCP_ERR_INVALID;
  }
  return PCP_OK;
}

}  // extern "C"
