// pcp_compare.hip -- map comparison on gfx950 ("Map comparison", MC1-MC9): per core point of the uploaded map, the
// signed distance along its oriented normal to an earlier survey (the base) inside a cylinder, with a level of detection from
// the two epochs' scatter (Lague et al.'s M3C2).  The rule is pcp_compare.hpp's: exact int64 sums over the candidates of each
// epoch, a fixed fp64 finish.
// Search: the cell-wave search of pcp_cell_search.hpp over ONE grid (cell >= search radius) for both clouds, the map's finite
// points first and the base's finite rows after them, the record's word the caller's index with the epoch in the top bit.
// The grid keeps the view's order inside a cell, so a cell's map records come before its base records: a work item is up to
// 64 MAP records of one cell, opened on map records only.  Both epochs are accumulated in the same walk, selected by the
// (wave-uniform) epoch bit.  MC5 / MC6 finish in the same kernel.
#include <algorithm>
#include <cmath>
#include <new>
#include <thread>
#include <vector>

#include "pcp_cell_search.hpp"
#include "pcp_device.hpp"
#include "pcp_internal.hpp"
#include "pcp_normals.hpp"
#include "pcp_compare.hpp"

namespace pcp {

constexpr uint32_t kMcEpochBit = 0x80000000u;
constexpr int64_t kMcMaxPoints = (int64_t(1) << 31) - 64;  // MC9: n + n_base

// the two clouds as one view: the map's finite points (tag = caller's index), then the base's finite rows (tag has the epoch bit)
__global__ __launch_bounds__(kCellBlock) void k_mc_concat(const float *__restrict__ ax, const float *__restrict__ ay,
                                                          const float *__restrict__ az, const int32_t *__restrict__ aremap,
                                                          int64_t ma, const float *__restrict__ bx, const float *__restrict__ by,
                                                          const float *__restrict__ bz, const uint32_t *__restrict__ btag, int64_t mb,
                                                          float *__restrict__ cx, float *__restrict__ cy, float *__restrict__ cz,
                                                          uint32_t *__restrict__ ctag) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x;
  if (k >= ma + mb) return;
  if (k < ma) {
    cx[k] = ax[k];
    cy[k] = ay[k];
    cz[k] = az[k];
    ctag[k] = static_cast<uint32_t>(aremap ? aremap[k] : static_cast<int32_t>(k));
  } else {
    const int64_t j = k - ma;
    cx[k] = bx[j];
    cy[k] = by[j];
    cz[k] = bz[j];
    ctag[k] = btag[j];
  }
}

// the record's word is the tag; only a map record opens a work item (a cell's map records come first)
struct McStage {
  const uint32_t *tag;
  __device__ uint32_t word(int64_t, int32_t v) const { return tag[v]; }
  __device__ bool opens(uint32_t w) const { return !(w & kMcEpochBit); }
};

// one work item: the map records k0 .. of one cell (up to kCellQ) against the records of the neighbouring cells.
// tally[0..5] += core, measured, positive, negative, no counterpart, too few own; tally[6] = max(candidates of one epoch):
// one atomic per counter per wavefront.
__global__ __launch_bounds__(kCellQ) void k_mc_compare(const uint4 *__restrict__ rec, const int32_t *__restrict__ items, GridDesc g,
                                                       const int32_t *__restrict__ start, mc::Rule rule,
                                                       const float *__restrict__ normals, int32_t normal_stride,
                                                       float *__restrict__ out_distance, float *__restrict__ out_lod,
                                                       uint8_t *__restrict__ out_status, long long *__restrict__ out_sums,
                                                       int32_t *__restrict__ out_direction, unsigned long long *__restrict__ tally) {
  const CellItem it = cell_open(rec, items, g, start);
  const int lane = threadIdx.x;
  const uint4 q = it.q;
  const bool query = lane < it.n && !(q.w & kMcEpochBit);  // (the cell's base records follow its map records)
  const float qx = __uint_as_float(q.x), qy = __uint_as_float(q.y), qz = __uint_as_float(q.z);
  const int64_t i = static_cast<int64_t>(q.w & ~kMcEpochBit);
  mc::Direction dir{};
  bool core = false;
  if (query) {
    const float *nrm = normals + i * normal_stride;
    core = mc::direction(rule, qx, qy, qz, nrm[0], nrm[1], nrm[2], dir);
  }
  mc::Sums su;
  mc::clear(su);
  const float t = rule.t;
  cell_walk(rec, g, start, it, core, [&](const uint4 &c) {
    // every operation rounded on its own (-ffp-contract=off); the integer part is 32 x 32 -> 64 multiply-adds
    mc::visit(su, dir, t, __uint_as_float(c.x) - qx, __uint_as_float(c.y) - qy, __uint_as_float(c.z) - qz, c.w >> 31);
  });
  // MC5 / MC6 (a core point is its own candidate in epoch A: nA >= 1)
  mc::Result res;
  res.distance = res.lod = 0.0f;
  res.status = mc::kNotCore;
  if (core) res = mc::finish(rule, dir, su);
  const unsigned long long v_core = __ballot(core), v_pos = __ballot(res.status == mc::kPositive),
                           v_neg = __ballot(res.status == mc::kNegative), v_meas = __ballot(res.status >= mc::kMeasured),
                           v_none = __ballot(res.status == mc::kNoCounterpart), v_few = __ballot(res.status == mc::kTooFewOwn);
  const uint32_t most = wave_max_u32(core ? static_cast<uint32_t>(max(su.nA, su.nB)) : 0u);  // (below 2^31: the clouds' size)
  if (lane == 0 && v_core) {
    atomicAdd(tally + 0, static_cast<unsigned long long>(__popcll(v_core)));
    if (v_meas) atomicAdd(tally + 1, static_cast<unsigned long long>(__popcll(v_meas)));
    if (v_pos) atomicAdd(tally + 2, static_cast<unsigned long long>(__popcll(v_pos)));
    if (v_neg) atomicAdd(tally + 3, static_cast<unsigned long long>(__popcll(v_neg)));
    if (v_none) atomicAdd(tally + 4, static_cast<unsigned long long>(__popcll(v_none)));
    if (v_few) atomicAdd(tally + 5, static_cast<unsigned long long>(__popcll(v_few)));
    atomicMax(tally + 6, static_cast<unsigned long long>(most));
  }
  if (!core) return;  // (the outputs were cleared: status 0 and zeros)
  out_distance[i] = res.distance;
  out_lod[i] = res.lod;
  out_status[i] = res.status;
  int64_t w[mc::kSumWords];
  mc::store(su, w);
#pragma unroll
  for (int a = 0; a < mc::kSumWords; ++a) out_sums[i * mc::kSumWords + a] = w[a];
  out_direction[3 * i + 0] = dir.N[0];
  out_direction[3 * i + 1] = dir.N[1];
  out_direction[3 * i + 2] = dir.N[2];
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// per-call scratch: released when the call returns
struct McScratch {
  FiniteScratch fin;
  DevBuf<float> cxyz, normals;
  DevBuf<uint32_t> ctag;
  DevBuf<uint8_t> flag;
  CellSearch search;
};

static int rule_of(const pcp_context *ctx, const char *who, const pcp_compare_params *p, mc::Rule *rule) {
  const char *why = mc::prepare(p->cyl_radius, p->cyl_half_length, p->reg_error, p->min_points, p->orient_mode, p->orient, rule);
  if (!why) return PCP_OK;
  if (ctx) return set_error(ctx, PCP_ERR_INVALID, "%s: %s (cyl_radius %g, cyl_half_length %g, reg_error %g, min_points %d, orient_mode %d)",
                            who, why, static_cast<double>(p->cyl_radius), static_cast<double>(p->cyl_half_length),
                            static_cast<double>(p->reg_error), p->min_points, p->orient_mode);
  set_global_error("%s: %s (cyl_radius %g, cyl_half_length %g, reg_error %g, min_points %d, orient_mode %d)", who, why,
                   static_cast<double>(p->cyl_radius), static_cast<double>(p->cyl_half_length), static_cast<double>(p->reg_error),
                   p->min_points, p->orient_mode);
  return PCP_ERR_INVALID;
}

// the ma > 0 finite map points of view cv and the base: one grid, records, work items, the search
static int compare_finite(pcp_context *ctx, const CloudView &cv, const mc::Rule &rule, const float *d_normals, int32_t normal_stride,
                          McScratch &s) {
  CompareState &cs = ctx->compare;
  const int64_t ma = cv.n, mb = cs.m_base, m = ma + mb;
  const size_t pm = (static_cast<size_t>(m) + 3) & ~size_t(3), pb = (static_cast<size_t>(mb) + 3) & ~size_t(3);
  PCP_HIP_TRY(ctx, s.cxyz.ensure(3 * pm + 4));
  PCP_HIP_TRY(ctx, s.ctag.ensure(static_cast<size_t>(m) + 4));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_mc_concat, dim3(cell_blocks(m)), dim3(kCellBlock), 0, ctx->stream, cv.x, cv.y, cv.z, cv.remap, ma, cs.base_xyz.p,
                       cs.base_xyz.p + pb, cs.base_xyz.p + 2 * pb, cs.base_tag.p, mb, s.cxyz.p, s.cxyz.p + pm, s.cxyz.p + 2 * pm,
                       s.ctag.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  CloudView both{};
  both.x = s.cxyz.p;
  both.y = s.cxyz.p + pm;
  both.z = s.cxyz.p + 2 * pm;
  both.n = m;
  both.remap = nullptr;
  for (int a = 0; a < 3; ++a) {  // the union of the boxes
    both.mn[a] = mb > 0 ? std::min(cv.mn[a], cs.mn[a]) : cv.mn[a];
    both.mx[a] = mb > 0 ? std::max(cv.mx[a], cs.mx[a]) : cv.mx[a];
  }
  CellSearch &search = s.search;
  int rc = cell_search_prepare(ctx, both, rule.search_radius, "pcp_compare", PCP_K_MISC, McStage{s.ctag.p}, ma, s.flag, search);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->s_counter.p, 0, 64, ctx->stream));  // (compact_flags left its total there)
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    if (search.n_items > 0)
      hipLaunchKernelGGL(k_mc_compare, dim3(static_cast<uint32_t>(search.n_items)), dim3(kCellQ), 0, ctx->stream, search.rec.p,
                         search.items.p, search.g, ctx->g_start.p, rule, d_normals, normal_stride, cs.distance.p, cs.lod.p,
                         cs.status.p, cs.sums.p, cs.direction.p, ctx->s_counter.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return PCP_OK;
}

static int compare_run(pcp_context *ctx, const mc::Rule &rule, const float *host_normals, int64_t out_stats[8]) {
  CompareState &cs = ctx->compare;
  const int64_t n = ctx->n;
  const size_t sn = static_cast<size_t>(n);
  cs.result_live = false;
  for (int a = 0; a < 8; ++a) cs.stats[a] = 0;
  PCP_HIP_TRY(ctx, cs.distance.ensure(sn + 4));
  PCP_HIP_TRY(ctx, cs.lod.ensure(sn + 4));
  PCP_HIP_TRY(ctx, cs.status.ensure(sn + 16));
  PCP_HIP_TRY(ctx, cs.sums.ensure(sn * mc::kSumWords + 4));
  PCP_HIP_TRY(ctx, cs.direction.ensure(3 * sn + 4));
  // MC1: a point that is not a core point keeps status 0 and zeros
  PCP_HIP_TRY(ctx, hipMemsetAsync(cs.distance.p, 0, (sn + 4) * 4, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(cs.lod.p, 0, (sn + 4) * 4, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(cs.status.p, 0, sn + 16, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(cs.sums.p, 0, (sn * mc::kSumWords + 4) * 8, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(cs.direction.p, 0, (3 * sn + 4) * 4, ctx->stream));
  McScratch s;
  const float *d_normals = ctx->gn_normal.p;
  int32_t normal_stride = 4;
  if (host_normals) {
    PCP_HIP_TRY(ctx, s.normals.ensure(3 * sn + 4));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(s.normals.p, host_normals, 3 * sn * 4, hipMemcpyHostToDevice, ctx->stream));
    d_normals = s.normals.p;
    normal_stride = 3;
  }
  CloudView cv;
  // MC1: the grid (which needs finite coordinates) is built over the finite points only
  int rc = finite_view(ctx, /*with_remap=*/true, /*timing_slot=*/-1, s.fin, &cv);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, ctx->s_counter.ensure(8));
  PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->s_counter.p, 0, 64, ctx->stream));
  if (cv.n > 0 && (rc = compare_finite(ctx, cv, rule, d_normals, normal_stride, s)) != PCP_OK) return rc;
  unsigned long long tally[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  PCP_HIP_TRY(ctx, hipMemcpyAsync(tally, ctx->s_counter.p, 64, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (also: the scratch is released on return)
  drop_large_grid_bitmap(ctx);
  if (static_cast<int64_t>(tally[6]) >= mc::kMaxCandidates)
    return set_error(ctx, PCP_ERR_RANGE, "pcp_compare: a point has %llu candidates in one epoch (2^22 or more could overflow the sums)",
                     tally[6]);
  for (int a = 0; a < 7; ++a) cs.stats[a] = static_cast<int64_t>(tally[a]);
  cs.stats[7] = 0;
  cs.n = n;
  cs.result_live = true;
  if (out_stats)
    for (int a = 0; a < 8; ++a) out_stats[a] = cs.stats[a];
  return PCP_OK;
}

// (pcp_create loads every code object of the library up front: see preload_code_objects in pcp_context.hip)
hipError_t preload_compare() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_mc_compare));
}

}  // namespace pcp

using namespace pcp;

extern "C" {

void pcp_default_compare_params(pcp_compare_params *p) {
  if (!p) return;
  p->cyl_radius = 0.03f;
  p->cyl_half_length = 0.05f;
  p->reg_error = 0.0f;
  p->min_points = 5;
  p->orient_mode = 0;
  p->orient[0] = p->orient[1] = p->orient[2] = 0.0f;
}

int pcp_compare_set_base(pcp_context *ctx, const void *points, int64_t n_base, int64_t stride_bytes) {
  if (!ctx) return PCP_ERR_INVALID;
  if (n_base < 0 || n_base > kMcMaxPoints || stride_bytes < 12 || (stride_bytes & 3) != 0 || (n_base > 0 && !points))
    return set_error(ctx, PCP_ERR_INVALID, "pcp_compare_set_base: n_base %lld outside 0..2^31-64, stride %lld not a multiple of 4 >= 12, or no rows",
                     static_cast<long long>(n_base), static_cast<long long>(stride_bytes));
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  CompareState &cs = ctx->compare;
  cs.base_live = false;
  cs.result_live = false;  // (a result belongs to the base it was made with)
  cs.reg.live = false;     // (RG1: so does a registration; the transform starts again at the identity)
  cs.coarse.release_base();  // (CG7: and the descriptors and normals of the old base's rows)
  // MC3: non-finite rows are never candidates -- they are left out here; the tag keeps the caller's row
  std::vector<float> planes;
  std::vector<uint32_t> tag;
  int64_t mb = 0;
  const unsigned char *rows = static_cast<const unsigned char *>(points);
  auto row = [&](int64_t j) { return reinterpret_cast<const float *>(rows + j * stride_bytes); };
  try {
    for (int64_t j = 0; j < n_base; ++j) mb += gn::finite3(row(j)[0], row(j)[1], row(j)[2]) ? 1 : 0;
    const size_t pb = (static_cast<size_t>(mb) + 3) & ~size_t(3);
    planes.assign(3 * pb + 4, 0.0f);
    tag.assign(static_cast<size_t>(mb) + 4, 0u);
    size_t k = 0;
    for (int a = 0; a < 3; ++a) cs.mn[a] = cs.mx[a] = 0.0f;
    for (int64_t j = 0; j < n_base; ++j) {
      const float *r = row(j);
      if (!gn::finite3(r[0], r[1], r[2])) continue;
      for (int a = 0; a < 3; ++a) {
        planes[static_cast<size_t>(a) * pb + k] = r[a];
        cs.mn[a] = k == 0 ? r[a] : std::min(cs.mn[a], r[a]);
        cs.mx[a] = k == 0 ? r[a] : std::max(cs.mx[a], r[a]);
      }
      tag[k] = static_cast<uint32_t>(j) | kMcEpochBit;
      ++k;
    }
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_compare_set_base: out of host memory for %lld rows", static_cast<long long>(n_base));
  }
  PCP_HIP_TRY(ctx, cs.base_xyz.ensure(planes.size()));
  PCP_HIP_TRY(ctx, cs.base_tag.ensure(tag.size()));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(cs.base_xyz.p, planes.data(), planes.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(cs.base_tag.p, tag.data(), tag.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  cs.n_base = n_base;
  cs.m_base = mb;
  cs.base_live = true;
  return PCP_OK;
}

int pcp_compare(pcp_context *ctx, const pcp_compare_params *p, const float *normals, int64_t out_stats[8]) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_stats)
    for (int a = 0; a < 8; ++a) out_stats[a] = 0;
  if (!p) return set_error(ctx, PCP_ERR_INVALID, "pcp_compare: no parameters");
  mc::Rule rule;
  int rc = rule_of(ctx, "pcp_compare", p, &rule);
  if (rc != PCP_OK) return rc;
  CompareState &cs = ctx->compare;
  if (!ctx->xyz.p) return set_error(ctx, PCP_ERR_STATE, "pcp_compare: no cloud uploaded");
  if (!cs.base_live) return set_error(ctx, PCP_ERR_STATE, "pcp_compare: no base (pcp_compare_set_base)");
  if (!normals && !ctx->gn_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_compare: no normals (pcp_estimate_normals on this cloud, or pass an array)");
  if (ctx->n + cs.n_base > kMcMaxPoints)
    return set_error(ctx, PCP_ERR_INVALID, "pcp_compare: %lld map points and %lld base rows are more than 2^31 - 64 together",
                     static_cast<long long>(ctx->n), static_cast<long long>(cs.n_base));
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->n == 0) {
    cs.result_live = true;
    cs.n = 0;
    for (int a = 0; a < 8; ++a) cs.stats[a] = 0;
    return PCP_OK;
  }
  return compare_run(ctx, rule, normals, out_stats);
}

int pcp_compare_fetch(pcp_context *ctx, float *out_distance, float *out_lod, uint8_t *out_status, int64_t *out_sums8,
                      int32_t *out_direction3) {
  if (!ctx) return PCP_ERR_INVALID;
  CompareState &cs = ctx->compare;
  if (!cs.result_live) return set_error(ctx, PCP_ERR_STATE, "pcp_compare_fetch: no result (pcp_compare on this cloud)");
  if (cs.n == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sn = static_cast<size_t>(cs.n);
  if (out_distance) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_distance, cs.distance.p, sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_lod) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_lod, cs.lod.p, sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_status) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_status, cs.status.p, sn, hipMemcpyDeviceToHost, ctx->stream));
  if (out_sums8) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_sums8, cs.sums.p, sn * mc::kSumWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out_direction3) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_direction3, cs.direction.p, 3 * sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

int pcp_compare_end(pcp_context *ctx) {
  if (!ctx) return PCP_ERR_INVALID;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->compare.release();
  return PCP_OK;
}

int pcp_compare_host(const pcp_compare_params *p, int64_t n, const float *xyz, const float *normals, int64_t n_base,
                     const float *base_xyz, float *out_distance, float *out_lod, uint8_t *out_status, int64_t *out_sums8,
                     int32_t *out_direction3, int64_t out_stats[8]) {
  if (out_stats)
    for (int a = 0; a < 8; ++a) out_stats[a] = 0;
  if (!p) {
    set_global_error("pcp_compare_host: no parameters");
    return PCP_ERR_INVALID;
  }
  mc::Rule rule;
  int rc = rule_of(nullptr, "pcp_compare_host", p, &rule);
  if (rc != PCP_OK) return rc;
  if (n < 0 || n > 65536 || n_base < 0 || n_base > 65536 || (n > 0 && (!xyz || !normals)) || (n_base > 0 && !base_xyz)) {
    set_global_error("pcp_compare_host: n or n_base outside 0..65536 or a missing array");
    return PCP_ERR_INVALID;
  }
  std::vector<int64_t> tallies(8 * 8, 0);  // per worker: the six counts, the most candidates, range violations
  auto rows = [&](int64_t i0, int64_t i1, int64_t *tally) {
    for (int64_t i = i0; i < i1; ++i) {
      mc::Result res;
      res.distance = res.lod = 0.0f;
      res.status = mc::kNotCore;
      mc::Sums su;
      mc::clear(su);
      mc::Direction dir{};
      const float qx = xyz[3 * i], qy = xyz[3 * i + 1], qz = xyz[3 * i + 2];
      const bool core = gn::finite3(qx, qy, qz) &&
                        mc::direction(rule, qx, qy, qz, normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], dir);
      if (core) {
        for (uint32_t epoch = 0; epoch < 2; ++epoch) {
          const float *pts = epoch ? base_xyz : xyz;
          const int64_t cnt = epoch ? n_base : n;
          for (int64_t j = 0; j < cnt; ++j) {
            const float cx = pts[3 * j], cy = pts[3 * j + 1], cz = pts[3 * j + 2];
            if (!gn::finite3(cx, cy, cz)) continue;
            const float dx = cx - qx, dy = cy - qy, dz = cz - qz;
            if ((dx * dx + dy * dy) + dz * dz <= rule.t &&
                !mc::bounds_hold(rule, dir, gn::quantise(dx), gn::quantise(dy), gn::quantise(dz)))
              tally[7] += 1;  // MC3's ranges: asserted, never seen
            mc::visit(su, dir, rule.t, dx, dy, dz, epoch);
          }
        }
        res = mc::finish(rule, dir, su);
        tally[0] += 1;
        tally[1] += res.status >= mc::kMeasured ? 1 : 0;
        tally[2] += res.status == mc::kPositive ? 1 : 0;
        tally[3] += res.status == mc::kNegative ? 1 : 0;
        tally[4] += res.status == mc::kNoCounterpart ? 1 : 0;
        tally[5] += res.status == mc::kTooFewOwn ? 1 : 0;
        tally[6] = std::max(tally[6], std::max(su.nA, su.nB));
      } else {
        mc::clear(su);
        dir.N[0] = dir.N[1] = dir.N[2] = 0;
      }
      if (out_distance) out_distance[i] = res.distance;
      if (out_lod) out_lod[i] = res.lod;
      if (out_status) out_status[i] = res.status;
      if (out_sums8) mc::store(su, out_sums8 + i * mc::kSumWords);
      if (out_direction3)
        for (int a = 0; a < 3; ++a) out_direction3[3 * i + a] = dir.N[a];
    }
  };
  // every query on its own (the rows do not interact): up to 8 host threads share them
  const int64_t workers = std::max<int64_t>(1, std::min<int64_t>({8, static_cast<int64_t>(std::thread::hardware_concurrency()), n / 1024}));
  std::vector<std::thread> pool;
  for (int64_t w = 1; w < workers; ++w) pool.emplace_back(rows, n * w / workers, n * (w + 1) / workers, tallies.data() + 8 * w);
  rows(0, n / workers, tallies.data());
  for (std::thread &th : pool) th.join();
  int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t w = 0; w < workers; ++w) {
    for (int a = 0; a < 6; ++a) stats[a] += tallies[static_cast<size_t>(8 * w + a)];
    stats[6] = std::max(stats[6], tallies[static_cast<size_t>(8 * w + 6)]);
    stats[7] += tallies[static_cast<size_t>(8 * w + 7)];
  }
  if (stats[7] != 0) {
    set_global_error("pcp_compare_host: %lld offsets left the ranges of MC3 (a defect of the rule)", static_cast<long long>(stats[7]));
    return PCP_ERR_RANGE;
  }
  // (2^22 candidates of one epoch cannot be reached with 65536 points)
  if (out_stats)
    for (int a = 0; a < 8; ++a) out_stats[a] = stats[a];
  return PCP_OK;
}

}  // extern "C"
