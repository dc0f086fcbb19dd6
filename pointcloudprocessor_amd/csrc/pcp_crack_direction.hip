// pcp_crack_direction.hip -- crack directions on the map ("Crack directions on the map", CD1-CD9): per crack point
// the exact integer moments of its links, the tangent they give and its anisotropy; per crack of pcp_crack_components the sums
// of those moments, from which the host takes the crack's axis.  The reference only blurs one keyframe's 2-D skeleton and looks
// at it (scripts/evalSkeletonDirection.py).
//
// The stage runs after the component stage for its parameters on that call's scratch: the crack points in cell order, the
// grid, the roots and their ranks.  One kernel, one lane per place of the cell order: the walk over the links of the place
// (crack_walk<false>, the cost class of k_cc_union) with the ten moments in registers, then the eigenpair and the per-point
// stores, then the row sums -- merged over the wavefront first where its live lanes share a crack, as the statistics kernels of
// the chain do.  Every sum is a 64-bit integer add, so the table does not depend on the order in which the lanes arrive.
#include <algorithm>
#include <new>
#include <vector>

#include "pcp_device.hpp"
#include "pcp_eigen33.hpp"
#include "pcp_crack_map.hpp"
#include "pcp_crack_direction.hpp"

namespace pcp {

constexpr int kCdBlock = 256;

static inline uint32_t cd_blocks(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kCdBlock))); }

// CD2-CD4.  tangent 3 n, anisotropy n, links n, moments 10 n (nullable): input order, zeroed by the caller.  table: rows of
// cd::kRowWords words, zeroed.  *over is raised where a point has gn::kMaxNeighbours links or more.
__global__ __launch_bounds__(kCdBlock) void k_cd_directions(const float *__restrict__ gx, const float *__restrict__ gy,
                                                            const float *__restrict__ gz, const int32_t *__restrict__ order, int64_t m,
                                                            GridDesc g, const int32_t *__restrict__ start, float t,
                                                            const int32_t *__restrict__ root_of, const int32_t *__restrict__ rank,
                                                            const int32_t *__restrict__ list, float *__restrict__ tangent,
                                                            float *__restrict__ anisotropy, int32_t *__restrict__ links,
                                                            long long *__restrict__ moments, unsigned long long *__restrict__ table,
                                                            uint32_t *__restrict__ over) {
  const int64_t s64 = static_cast<int64_t>(blockIdx.x) * kCdBlock + threadIdx.x;
  const bool valid = s64 < m;
  gn::Moments mo;
  gn::clear(mo);
  int32_t row = -1;
  if (valid) {
    const int32_t s = static_cast<int32_t>(s64);
    const float qx = gx[s], qy = gy[s], qz = gz[s];
    // CD1: d = fl32(p_j - p_i), the test of CC2 on it, then the integer adds
    crack_walk<false>(g, start, qx, qy, qz, s, m, [&](int32_t c) { gn::visit(mo, gx[c] - qx, gy[c] - qy, gz[c] - qz, t); });
    const int32_t k = order[s];
    row = rank[root_of[k]];
    const int64_t i = list[k];
    if (mo.n >= gn::kMaxNeighbours) atomicMax(over, 1u);
    // CD3
    float tx = 0.0f, ty = 0.0f, tz = 0.0f, an = 0.0f;
    if (mo.n >= cd::kMinLinks) {
      double C[6], M[6], ev, v[3];
      gn::covariance(mo, C);
      const double trace = cd::trace_of(C);
      if (trace > 0.0) {
        cd::flipped(C, trace, M);
        smallest_eigenpair(M, ev, v);
        const double l1 = trace - ev;
        if (l1 > 0.0) {
          if (!cd::unit_ok(v)) cd::degenerate_vector(M, ev, v);
          cd::orient(v);
          tx = static_cast<float>(v[0]);
          ty = static_cast<float>(v[1]);
          tz = static_cast<float>(v[2]);
          an = static_cast<float>(l1 / trace);
        }
      }
    }
    tangent[3 * i + 0] = tx;
    tangent[3 * i + 1] = ty;
    tangent[3 * i + 2] = tz;
    anisotropy[i] = an;
    links[i] = static_cast<int32_t>(mo.n);
    if (moments) {
      int64_t w[gn::kMomentWords];
      gn::store(mo, w);
#pragma unroll
      for (int a = 0; a < gn::kMomentWords; ++a) moments[i * gn::kMomentWords + a] = w[a];
    }
  }
  // CD4 (a lane beyond m holds zeros)
  bool shared;
  const bool issue = wave_row_issuer(valid, row, &shared);
  int64_t w[gn::kMomentWords];
  gn::store(mo, w);
  unsigned long long *out = table + static_cast<int64_t>(cd::kRowWords) * (issue ? row : 0);
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

hipError_t preload_crack_direction() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_cd_directions));
}

// the m > 0 crack points and rows > 0 cracks the component stage left in cc and ctx->g_*
static int crack_directions_run(pcp_context *ctx, const pcp_crack_link_params &p, const CcScratch &cc, CdScratch &s, bool with_moments,
                                const CrackCounts &c) {
  CrackMap &cm = *ctx->crack;
  const int64_t m = c.points;
  const size_t sn = static_cast<size_t>(ctx->n), pm = (static_cast<size_t>(m) + 3) & ~size_t(3);
  const float *gx = ctx->g_xyz.p, *gy = ctx->g_xyz.p + pm, *gz = ctx->g_xyz.p + 2 * pm;
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cd_directions, dim3(cd_blocks(m)), dim3(kCdBlock), 0, ctx->stream, gx, gy, gz, ctx->g_order.p, m, cc.grid,
                       ctx->g_start.p, gn::threshold_of(p.radius), cc.root_of.p, cc.rank.p, cc.list.p, s.f32.p, s.f32.p + 3 * sn, s.links.p,
                       with_moments ? s.moments.p : nullptr, cm.cd_table.p, s.words.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  uint32_t over = 0;
  PCP_HIP_TRY(ctx, hipMemcpyAsync(&over, s.words.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (over)
    return set_error(ctx, PCP_ERR_RANGE, "pcp_crack_directions: a crack point has %lld links or more", static_cast<long long>(gn::kMaxNeighbours));
  return PCP_OK;
}

struct CdOut {
  float *tangent, *anisotropy;
  int32_t *links;
  int64_t *moments;
};

// the component stage, the direction stage and the copies of the per-point outputs, queued
static int crack_direction_stages(pcp_context *ctx, const pcp_crack_link_params &p, const CdOut &out, CcScratch &cc, CdScratch &s,
                                  CrackCounts *c) {
  CrackMap &cm = *ctx->crack;
  const size_t sn = static_cast<size_t>(ctx->n);
  int rc = crack_components_run(ctx, p, cc, c);
  if (rc != PCP_OK) return rc;
  const size_t sr = static_cast<size_t>(c->cracks);
  PCP_HIP_TRY(ctx, s.f32.ensure(4 * sn + 4));
  PCP_HIP_TRY(ctx, s.links.ensure(sn + 4));
  PCP_HIP_TRY(ctx, s.words.ensure(4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.f32.p, 0, 4 * sn * 4, ctx->stream));  // CD2, CD3: zeros for a point that is no crack point
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.links.p, 0, sn * 4, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.words.p, 0, 16, ctx->stream));
  if (out.moments) {
    PCP_HIP_TRY(ctx, s.moments.ensure(static_cast<size_t>(gn::kMomentWords) * sn + 4));
    PCP_HIP_TRY(ctx, hipMemsetAsync(s.moments.p, 0, static_cast<size_t>(gn::kMomentWords) * sn * 8, ctx->stream));
  }
  PCP_HIP_TRY(ctx, cm.cd_ids.ensure(sr + 4));
  PCP_HIP_TRY(ctx, cm.cd_table.ensure(static_cast<size_t>(cd::kRowWords) * sr + 4));
  if (c->points > 0) {
    PCP_HIP_TRY(ctx, hipMemcpyAsync(cm.cd_ids.p, cm.cc_ids.p, sr * 4, hipMemcpyDeviceToDevice, ctx->stream));
    PCP_HIP_TRY(ctx, hipMemsetAsync(cm.cd_table.p, 0, static_cast<size_t>(cd::kRowWords) * sr * 8, ctx->stream));
    if ((rc = crack_directions_run(ctx, p, cc, s, out.moments != nullptr, *c)) != PCP_OK) return rc;
  }
  if (out.tangent) PCP_HIP_TRY(ctx, hipMemcpyAsync(out.tangent, s.f32.p, 3 * sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out.anisotropy) PCP_HIP_TRY(ctx, hipMemcpyAsync(out.anisotropy, s.f32.p + 3 * sn, sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out.links) PCP_HIP_TRY(ctx, hipMemcpyAsync(out.links, s.links.p, sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out.moments)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out.moments, s.moments.p, static_cast<size_t>(gn::kMomentWords) * sn * 8, hipMemcpyDeviceToHost, ctx->stream));
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_crack_directions(pcp_context *ctx, const pcp_crack_link_params *p, float *out_tangent, float *out_anisotropy, int32_t *out_links,
                         int64_t *out_moments, int64_t *out_crack_points, int64_t *out_cracks) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_crack_points) *out_crack_points = 0;
  if (out_cracks) *out_cracks = 0;
  int rc = crack_link_check(ctx, "pcp_crack_directions", p);
  if (rc != PCP_OK) return rc;
  // CD1, CD6: towards the chain's state the call is a pcp_crack_components that also makes the directions
  CrackMap &cm = *ctx->crack;
  CrackCounts c;
  cm.replacing(CrackMap::kComponents);
  cm.replacing_directions();
  if (ctx->n == 0) {
    cm.hold(CrackMap::kComponents, c);
    cm.hold_directions(0);
    return PCP_OK;
  }
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  CcScratch cc;
  CdScratch cd;
  const CdOut out{out_tangent, out_anisotropy, out_links, out_moments};
  rc = crack_direction_stages(ctx, *p, out, cc, cd, &c);
  const hipError_t e = hipStreamSynchronize(ctx->stream);  // (also: the scratch is released on return)
  drop_large_grid_bitmap(ctx);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, e);
  cm.hold(CrackMap::kComponents, c);
  cm.hold_directions(c.cracks);
  if (out_crack_points) *out_crack_points = c.points;
  if (out_cracks) *out_cracks = c.cracks;
  return PCP_OK;
}

int pcp_crack_directions_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows20, int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  const CrackMap &cm = *ctx->crack;
  int64_t rows = 0;
  const int rc = crack_window(ctx, "pcp_crack_directions_fetch", CrackMap::kDirections, first, max_rows, cm.cd_rows, &rows);
  if (rc != PCP_OK || rows == 0) return rc;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sr = static_cast<size_t>(rows), sf = static_cast<size_t>(first);
  if (out_id) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_id, cm.cd_ids.p + sf, sr * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_rows20)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rows20, cm.cd_table.p + cd::kRowWords * sf, cd::kRowWords * sr * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_crack_directions_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, float *out_tangent,
                              float *out_anisotropy, int32_t *out_links, int64_t *out_moments, int32_t *out_id, int64_t *out_rows20,
                              int64_t *out_cracks) {
  if (out_cracks) *out_cracks = 0;
  if (!cf::min_views_ok(min_views) || !gn::radius_ok(radius)) {
    set_global_error("pcp_crack_directions_host: min_views %d outside %d..%d or radius %g outside [0.005, 1]", min_views, cf::kMinViewsLo,
                     cf::kMinViewsHi, static_cast<double>(radius));
    return PCP_ERR_INVALID;
  }
  if (n < 0 || n > cf::kHostMaxPoints || (n > 0 && (!xyz || !views))) {
    set_global_error("pcp_crack_directions_host: n outside 0..65536 or a missing array");
    return PCP_ERR_INVALID;
  }
  cd::HostResult res;
  try {
    if (!cd::directions_brute(n, xyz, views, min_views, gn::threshold_of(radius), res)) {  // (cannot be with n <= 65536)
      set_global_error("pcp_crack_directions_host: a crack point has %lld links or more", static_cast<long long>(gn::kMaxNeighbours));
      return PCP_ERR_RANGE;
    }
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_crack_directions_host: out of host memory for %lld points", static_cast<long long>(n));
    return PCP_ERR_NOMEM;
  }
  if (out_tangent) std::copy(res.tangent.begin(), res.tangent.end(), out_tangent);
  if (out_anisotropy) std::copy(res.anisotropy.begin(), res.anisotropy.end(), out_anisotropy);
  if (out_links) std::copy(res.links.begin(), res.links.end(), out_links);
  if (out_moments) std::copy(res.moments.begin(), res.moments.end(), out_moments);
  if (out_id) std::copy(res.ids.begin(), res.ids.end(), out_id);
  if (out_rows20) std::copy(res.rows.begin(), res.rows.end(), out_rows20);
  if (out_cracks) *out_cracks = static_cast<int64_t>(res.ids.size());
  return PCP_OK;
}

int pcp_crack_axis_host(const int64_t row20[20], double out5[5]) {
  if (!row20 || !out5) {
    set_global_error("pcp_crack_axis_host: a NULL argument");
    return PCP_ERR_INVALID;
  }
  cd::axis_host(row20, out5);
  return PCP_OK;
}

}  // extern "C"
