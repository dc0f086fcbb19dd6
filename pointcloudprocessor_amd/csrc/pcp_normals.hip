// pcp_normals.hip -- geometry maps on gfx950 ("Geometry maps"): a normal per point of the uploaded map
// (pcp_estimate_normals, rules GN1-GN7) and the per-pixel range / camera position / camera normal / index images of one
// keyframe (pcp_frame_geometry, rules GM1-GM5) -- what scripts/genNormAndDistanceMask.py (class Crack, generate_norm_masks
// :200-231, generate_distance_masks :233-266) scatters on the host, one point at a time, from the per-keyframe clouds.
//
// Normals: the finite points are both queries and candidates; j is a neighbour of i iff the fp32 squared distance is <= t
// (LS2's threshold); each accepted offset is quantised to 2^-20 m and the ten moments about the query are exact int64 sums
// (pcp_normals.hpp), so they do not depend on the order of the neighbours, the grid or the input order.  The covariance is
// three fp64 operations per entry, the normal pcl::eigen33's smallest eigenvector (pcp_eigen33.hpp).
// Search: the cell-wave search of pcp_cell_search.hpp over the finite points, the record's word the caller's index.
//
// Maps: the contributors are the list pcp_frame_visible reports; each issues one 64-bit atomicMin of
// (range bits << 32 | input index) on its colour pixel, so the nearest point wins, ties go to the lowest index, and the
// result does not depend on the arrival order.  A resolve kernel, one lane per pixel, writes the four images.
#include <algorithm>
#include <cmath>
#include <new>
#include <thread>
#include <vector>

#include "pcp_cell_search.hpp"
#include "pcp_device.hpp"
#include "pcp_eigen33.hpp"
#include "pcp_eigen33_selftest.hpp"
#include "pcp_internal.hpp"
#include "pcp_normals.hpp"

namespace pcp {

// the record's word is the caller's index the result goes to
struct GnStage {
  const int32_t *remap;
  __device__ uint32_t word(int64_t, int32_t v) const { return static_cast<uint32_t>(remap[v]); }
  __device__ bool opens(uint32_t) const { return true; }
};

// one work item: the queries k0 .. k0 + n - 1 of one cell against the records of the neighbouring cells.
// tally[0] += valid points, tally[1] = max(tally[1], neighbour count): one atomic of each per wavefront.
__global__ __launch_bounds__(kCellQ) void k_gn_normals(const uint4 *__restrict__ rec, const int32_t *__restrict__ items, GridDesc g,
                                                       const int32_t *__restrict__ start, float t, float4 *__restrict__ out_normal,
                                                       int32_t *__restrict__ out_count, long long *__restrict__ out_moments,
                                                       unsigned long long *__restrict__ tally) {
  const CellItem it = cell_open(rec, items, g, start);
  const int lane = threadIdx.x;
  const bool active = lane < it.n;
  const uint4 q = it.q;
  const float qx = __uint_as_float(q.x), qy = __uint_as_float(q.y), qz = __uint_as_float(q.z);
  gn::Moments mo;
  gn::clear(mo);
  cell_walk(rec, g, start, it, active, [&](const uint4 &c) {
    // every operation rounded on its own (-ffp-contract=off); the S2 terms are 32 x 32 -> 64 multiply-adds
    gn::visit(mo, __uint_as_float(c.x) - qx, __uint_as_float(c.y) - qy, __uint_as_float(c.z) - qz, t);
  });
  // GN5-GN7 (an active query is its own neighbour: n >= 1)
  float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  bool valid = false;
  if (active) {
    double C[6], ev, nrm[3];
    gn::covariance(mo, C);
    smallest_eigenpair(C, ev, nrm);
    const double trace = (C[0] + C[3]) + C[5];
    const float nx = static_cast<float>(nrm[0]), ny = static_cast<float>(nrm[1]), nz = static_cast<float>(nrm[2]);
    valid = mo.n >= gn::kMinNeighbours && gn::finite3(nx, ny, nz);
    if (valid) res = make_float4(nx, ny, nz, trace > 0.0 ? static_cast<float>(ev / trace) : 0.0f);
  }
  const unsigned long long votes = __ballot(valid);
  uint32_t most = active ? static_cast<uint32_t>(mo.n) : 0u;  // (below 2^31: the cloud's size)
  for (int o = 32; o >= 1; o >>= 1) most = max(most, static_cast<uint32_t>(__shfl_xor(static_cast<int>(most), o, 64)));
  if (lane == 0) {
    if (votes) atomicAdd(tally, static_cast<unsigned long long>(__popcll(votes)));
    atomicMax(tally + 1, static_cast<unsigned long long>(most));
  }
  if (!active) return;
  const int64_t i = static_cast<int64_t>(q.w);
  out_normal[i] = res;
  out_count[i] = static_cast<int32_t>(mo.n);
  if (out_moments) {
    int64_t w[gn::kMomentWords];
    gn::store(mo, w);
#pragma unroll
    for (int a = 0; a < gn::kMomentWords; ++a) out_moments[i * gn::kMomentWords + a] = w[a];
  }
}

// pcp_selftest_eigen33, form 0: the solver and the two reciprocals as k_gn_normals above compiles them (no contraction: the
// flags of the build; pcp_crack_width.hip and pcp_crack_direction.hip include the same text under the same flags), one lane
// per item
__global__ __launch_bounds__(kCellBlock) void k_selftest_eigen33_plain(Eigen33SelftestArgs a) {
  eigen33_selftest_lane(a, static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x);
}

// ---- geometry maps ------------------------------------------------------------------------------------------------------
constexpr unsigned long long kGmEmpty = ~0ull;

__global__ __launch_bounds__(kCellBlock) void k_gm_clear(unsigned long long *__restrict__ keys, int64_t px) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x;
  if (p < px) keys[p] = kGmEmpty;
}

// GM2: one atomicMin per contributor (the list of pcp_frame_visible: every entry has a colour pixel; the test stays as a bound)
__global__ __launch_bounds__(kCellBlock) void k_gm_scatter(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ z, DevCamera cam, DevFrame fr,
                                                           const int32_t *__restrict__ index, int64_t m, int64_t px,
                                                           unsigned long long *__restrict__ keys) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x;
  if (k >= m) return;
  const int32_t i = index[k];
  const Projected p = project_point(cam, fr.w2c, x[i], y[i], z[i]);
  if (p.pixel < 0 || p.pixel >= px) return;
  const float range = static_cast<float>(range64(p.xc, p.yc, p.zc));  // what pcp_project_frame reports; positive: bits order as values
  atomicMin(keys + p.pixel, (static_cast<unsigned long long>(__float_as_uint(range)) << 32) | static_cast<uint32_t>(i));
}

// GM3 / GM4: one lane per pixel; *occupied += pixels with a winner (one atomic per wavefront)
__global__ __launch_bounds__(kCellBlock) void k_gm_resolve(const unsigned long long *__restrict__ keys, int64_t px,
                                                           const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ z, DevFrame fr,
                                                           const float4 *__restrict__ normals, int32_t *__restrict__ out_index,
                                                           float *__restrict__ out_range, float *__restrict__ out_xyz,
                                                           float *__restrict__ out_normal, unsigned long long *__restrict__ occupied) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x;
  bool hit = false;
  if (p < px) {
    const unsigned long long key = keys[p];
    hit = key != kGmEmpty;
    int32_t idx = -1;
    float range = 0.0f, xc = 0.0f, yc = 0.0f, zc = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (hit) {
      idx = static_cast<int32_t>(static_cast<uint32_t>(key));
      range = __uint_as_float(static_cast<uint32_t>(key >> 32));
      xform(fr.w2c, x[idx], y[idx], z[idx], xc, yc, zc);
      if (normals) {
        const float4 n = normals[idx];
        if (n.x != 0.0f || n.y != 0.0f || n.z != 0.0f) {  // (an invalid normal stays (0, 0, 0))
          const float *m = fr.w2c;  // xform's association without the translation
          nx = n.x * m[0] + (n.y * m[1] + n.z * m[2]);
          ny = n.x * m[4] + (n.y * m[5] + n.z * m[6]);
          nz = n.x * m[8] + (n.y * m[9] + n.z * m[10]);
          if ((nx * xc + ny * yc) + nz * zc > 0.0f) {  // faces away from the camera
            nx = -nx;
            ny = -ny;
            nz = -nz;
          }
        }
      }
    }
    out_index[p] = idx;
    out_range[p] = range;
    out_xyz[3 * p + 0] = xc;
    out_xyz[3 * p + 1] = yc;
    out_xyz[3 * p + 2] = zc;
    out_normal[3 * p + 0] = nx;
    out_normal[3 * p + 1] = ny;
    out_normal[3 * p + 2] = nz;
  }
  const unsigned long long votes = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(occupied, static_cast<unsigned long long>(__popcll(votes)));
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// per-call scratch: released when the call returns
struct GnScratch {
  FiniteScratch fin;  // (its flags serve the work items once the view is gathered)
  CellSearch search;
  DevBuf<long long> moments;
};

void normals_release(pcp_context *ctx) {
  ctx->gn_live = false;
  ctx->facets.release();  // FA9: the facets are made from these normals
  ctx->gn_normal.release();
  ctx->gn_count.release();
}

// the m > 0 finite points of view cv: the search's records and work items, the moments (nullable) and the solve into the
// caller's arrays under the view's remap.  s_counter is cleared first (compact_flags left its total there) and holds the tally.
static int normals_finite(pcp_context *ctx, const CloudView &cv, float radius, const char *who, DevBuf<uint8_t> &flag, CellSearch &cs,
                          float *out_normal4, int32_t *out_count, long long *out_moments) {
  int rc = cell_search_prepare(ctx, cv, radius, who, PCP_K_MISC, GnStage{cv.remap}, cv.n, flag, cs);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->s_counter.p, 0, 16, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    if (cs.n_items > 0)
      hipLaunchKernelGGL(k_gn_normals, dim3(static_cast<uint32_t>(cs.n_items)), dim3(kCellQ), 0, ctx->stream, cs.rec.p, cs.items.p,
                         cs.g, ctx->g_start.p, gn::threshold_of(radius), reinterpret_cast<float4 *>(out_normal4), out_count, out_moments,
                         ctx->s_counter.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return PCP_OK;
}

// CG1 (pcp_coarse.hip): the same search, moments and solve over a view that is not the uploaded map (cv.n > 0, cv.remap set);
// the results go to the caller's arrays and the map's live estimate stays as it is
int normals_of_view(pcp_context *ctx, const CloudView &cv, float radius, const char *who, float *out_normal4, int32_t *out_count,
                    int64_t *out_most) {
  DevBuf<uint8_t> flag;
  CellSearch cs;
  PCP_HIP_TRY(ctx, ctx->s_counter.ensure(4));
  int rc = normals_finite(ctx, cv, radius, who, flag, cs, out_normal4, out_count, nullptr);
  if (rc != PCP_OK) return rc;
  unsigned long long tally[2] = {0, 0};
  PCP_HIP_TRY(ctx, hipMemcpyAsync(tally, ctx->s_counter.p, 16, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (also: the search's scratch is released on return)
  drop_large_grid_bitmap(ctx);
  if (out_most) *out_most = static_cast<int64_t>(tally[1]);
  return PCP_OK;
}

static int estimate_normals(pcp_context *ctx, float radius, int64_t *out_valid, int64_t *out_moments) {
  const int64_t n = ctx->n;
  const size_t sn = static_cast<size_t>(n);
  ctx->gn_live = false;
  PCP_HIP_TRY(ctx, ctx->gn_normal.ensure(4 * sn + 4));
  PCP_HIP_TRY(ctx, ctx->gn_count.ensure(sn + 4));
  // GN7: a point that is not a query (non-finite) keeps normal (0, 0, 0), curvature 0, count 0
  PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->gn_normal.p, 0, (4 * sn + 4) * 4, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->gn_count.p, 0, (sn + 4) * 4, ctx->stream));
  GnScratch s;
  if (out_moments) {
    PCP_HIP_TRY(ctx, s.moments.ensure(sn * gn::kMomentWords + 4));
    PCP_HIP_TRY(ctx, hipMemsetAsync(s.moments.p, 0, sn * gn::kMomentWords * 8, ctx->stream));
  }
  CloudView cv;
  // GN1: the grid (which needs finite coordinates) is built over the finite points only
  int rc = finite_view(ctx, /*with_remap=*/true, /*timing_slot=*/-1, s.fin, &cv);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, ctx->s_counter.ensure(4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->s_counter.p, 0, 16, ctx->stream));
  if (cv.n > 0 && (rc = normals_finite(ctx, cv, radius, "pcp_estimate_normals", s.fin.flag, s.search, ctx->gn_normal.p, ctx->gn_count.p,
                                       s.moments.p)) != PCP_OK)
    return rc;
  unsigned long long tally[2] = {0, 0};
  PCP_HIP_TRY(ctx, hipMemcpyAsync(tally, ctx->s_counter.p, 16, hipMemcpyDeviceToHost, ctx->stream));
  if (out_moments)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_moments, s.moments.p, sn * gn::kMomentWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (also: the scratch is released on return)
  drop_large_grid_bitmap(ctx);  // (a tiny radius on a large map may take the sparse grid)
  if (static_cast<int64_t>(tally[1]) >= gn::kMaxNeighbours)
    return set_error(ctx, PCP_ERR_RANGE, "pcp_estimate_normals: a point has %llu neighbours within %g (2^22 or more could overflow the moments)",
                     tally[1], static_cast<double>(radius));
  ctx->gn_live = true;
  ctx->gn_radius = radius;
  if (out_valid) *out_valid = static_cast<int64_t>(tally[0]);
  return PCP_OK;
}

// The device part of pcp_frame_geometry, for the stages that read the maps where they are (pcp_crack_width.hip): the checks
// of frame_contributors under the caller's name, then the three kernels.  The images stay in ctx->gm_out (index | range |
// xyz_cam | normal_cam), the occupied count in ctx->s_counter[0]; nothing is copied and the stream is not synchronised.
// with_normals needs a live estimate (the caller's to check).
int frame_geometry_device(pcp_context *ctx, const char *who, int32_t frame, bool with_normals, int64_t *out_contributors) {
  int64_t m = 0;
  int rc = frame_contributors(ctx, who, frame, &m);  // GM1: the list of pcp_frame_visible, in ctx->s_cell
  if (rc != PCP_OK) return rc;
  if (out_contributors) *out_contributors = m;
  const int64_t px = static_cast<int64_t>(ctx->dcam.img_w) * ctx->dcam.img_h;
  if (px <= 0) return PCP_OK;
  const size_t spx = static_cast<size_t>(px);
  PCP_HIP_TRY(ctx, ctx->gm_keys.ensure(spx + 4));
  PCP_HIP_TRY(ctx, ctx->gm_out.ensure(8 * spx + 4));
  PCP_HIP_TRY(ctx, ctx->s_counter.ensure(4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->s_counter.p, 0, 8, ctx->stream));
  const size_t plane = (static_cast<size_t>(ctx->n) + 3) & ~size_t(3);
  const float *x = ctx->xyz.p, *y = ctx->xyz.p + plane, *z = ctx->xyz.p + 2 * plane;
  int32_t *d_index = reinterpret_cast<int32_t *>(ctx->gm_out.p);
  float *d_range = reinterpret_cast<float *>(ctx->gm_out.p + spx);
  float *d_xyz = reinterpret_cast<float *>(ctx->gm_out.p + 2 * spx);
  float *d_normal = reinterpret_cast<float *>(ctx->gm_out.p + 5 * spx);
  const DevFrame &fr = ctx->hframes[static_cast<size_t>(frame)];
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_gm_clear, dim3(cell_blocks(px)), dim3(kCellBlock), 0, ctx->stream, ctx->gm_keys.p, px);
    if (m > 0)
      hipLaunchKernelGGL(k_gm_scatter, dim3(cell_blocks(m)), dim3(kCellBlock), 0, ctx->stream, x, y, z, ctx->dcam, fr, ctx->s_cell.p, m, px,
                         ctx->gm_keys.p);
    hipLaunchKernelGGL(k_gm_resolve, dim3(cell_blocks(px)), dim3(kCellBlock), 0, ctx->stream, ctx->gm_keys.p, px, x, y, z, fr,
                       with_normals ? reinterpret_cast<const float4 *>(ctx->gn_normal.p) : nullptr, d_index, d_range, d_xyz,
                       d_normal, ctx->s_counter.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return PCP_OK;
}

// (pcp_create loads every code object of the library up front: see preload_code_objects in pcp_context.hip)
hipError_t preload_normals() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_gn_normals));
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_estimate_normals(pcp_context *ctx, float radius, int64_t *out_valid, int64_t *out_moments) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_valid) *out_valid = 0;
  if (!gn::radius_ok(radius))
    return set_error(ctx, PCP_ERR_INVALID, "pcp_estimate_normals: radius %g outside [0.005, 1]", static_cast<double>(radius));
  if (!ctx->xyz.p && ctx->n > 0) return set_error(ctx, PCP_ERR_STATE, "pcp_estimate_normals: no cloud uploaded");
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->facets.release();  // FA9: a new estimate ends the facets of the old one
  ctx->compare.coarse.release_map();  // CG7: and the map's descriptors, whose axes may have been the old one's
  if (ctx->n == 0) {
    ctx->gn_live = true;
    ctx->gn_radius = radius;
    return PCP_OK;
  }
  return estimate_normals(ctx, radius, out_valid, out_moments);
}

int pcp_normals_fetch(pcp_context *ctx, float *out_normal, float *out_curvature, int32_t *out_neighbours) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!ctx->gn_live) return set_error(ctx, PCP_ERR_STATE, "pcp_normals_fetch: pcp_estimate_normals has not run on this cloud");
  const int64_t n = ctx->n;
  if (n == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sn = static_cast<size_t>(n);
  std::vector<float> rows;
  if (out_normal || out_curvature) {
    try {
      rows.resize(4 * sn);
    } catch (const std::bad_alloc &) {
      return set_error(ctx, PCP_ERR_NOMEM, "pcp_normals_fetch: out of host memory for %lld points", static_cast<long long>(n));
    }
    PCP_HIP_TRY(ctx, hipMemcpyAsync(rows.data(), ctx->gn_normal.p, 4 * sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (out_neighbours) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_neighbours, ctx->gn_count.p, sn * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < sn && !rows.empty(); ++i) {
    if (out_normal) {
      out_normal[3 * i + 0] = rows[4 * i + 0];
      out_normal[3 * i + 1] = rows[4 * i + 1];
      out_normal[3 * i + 2] = rows[4 * i + 2];
    }
    if (out_curvature) out_curvature[i] = rows[4 * i + 3];
  }
  return PCP_OK;
}

int pcp_selftest_eigen33(pcp_context *ctx, int32_t form, int64_t n, const double *matrices, double *out_ev, double *out_vec, int64_t m,
                         const double *args, double *out_rcp, double *out_rsqrt) {
  if (!ctx) return PCP_ERR_INVALID;
  if (form != 0 && form != 1) return set_error(ctx, PCP_ERR_INVALID, "pcp_selftest_eigen33: form %d is neither 0 nor 1", static_cast<int>(form));
  constexpr int64_t kMost = int64_t(1) << 27;  // (the grid of one launch and a few GB of scratch)
  if (n < 0 || m < 0 || n > kMost || m > kMost)
    return set_error(ctx, PCP_ERR_INVALID, "pcp_selftest_eigen33: a count outside 0..2^27 (%lld matrices, %lld arguments)",
                     static_cast<long long>(n), static_cast<long long>(m));
  if (n > 0 && (!matrices || !out_ev || !out_vec)) return set_error(ctx, PCP_ERR_INVALID, "pcp_selftest_eigen33: %lld matrices and a missing array", static_cast<long long>(n));
  if (m > 0 && (!args || !out_rcp || !out_rsqrt)) return set_error(ctx, PCP_ERR_INVALID, "pcp_selftest_eigen33: %lld arguments and a missing array", static_cast<long long>(m));
  if (n == 0 && m == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // per-call scratch, released on return: in (6 n | m), out (n | 3 n | m | m); nothing of the context's is touched
  const size_t sn = static_cast<size_t>(n), sm = static_cast<size_t>(m);
  DevBuf<double> in, out;
  PCP_HIP_TRY(ctx, in.ensure(6 * sn + sm));
  PCP_HIP_TRY(ctx, out.ensure(4 * sn + 2 * sm));
  if (n > 0) PCP_HIP_TRY(ctx, hipMemcpyAsync(in.p, matrices, 6 * sn * 8, hipMemcpyHostToDevice, ctx->stream));
  if (m > 0) PCP_HIP_TRY(ctx, hipMemcpyAsync(in.p + 6 * sn, args, sm * 8, hipMemcpyHostToDevice, ctx->stream));
  Eigen33SelftestArgs a;
  a.mat = in.p;
  a.ev = out.p;
  a.vec = out.p + sn;
  a.n = n;
  a.arg = in.p + 6 * sn;
  a.rcp = out.p + 4 * sn;
  a.rsqrt = out.p + 4 * sn + sm;
  a.m = m;
  if (form == 0)
    hipLaunchKernelGGL(k_selftest_eigen33_plain, dim3(cell_blocks(std::max(n, m))), dim3(kCellBlock), 0, ctx->stream, a);
  else
    selftest_eigen33_launch_contracted(a, ctx->stream);
  PCP_HIP_TRY(ctx, hipGetLastError());
  if (n > 0) {
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_ev, a.ev, sn * 8, hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_vec, a.vec, 3 * sn * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (m > 0) {
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rcp, a.rcp, sm * 8, hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rsqrt, a.rsqrt, sm * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

int pcp_normals_moments_host(float radius, int64_t n, const float *xyz, int64_t *out_moments) {
  if (!gn::radius_ok(radius)) {
    set_global_error("pcp_normals_moments_host: radius %g outside [0.005, 1]", static_cast<double>(radius));
    return PCP_ERR_INVALID;
  }
  if (n < 0 || n > 65536 || (n > 0 && (!xyz || !out_moments))) {
    set_global_error("pcp_normals_moments_host: n outside 0..65536 or a missing array");
    return PCP_ERR_INVALID;
  }
  const float t = gn::threshold_of(radius);
  // every query on its own (the rows do not interact): up to 8 host threads share them
  auto rows = [=](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      gn::Moments mo;
      gn::clear(mo);
      const float qx = xyz[3 * i], qy = xyz[3 * i + 1], qz = xyz[3 * i + 2];
      if (gn::finite3(qx, qy, qz))
        for (int64_t j = 0; j < n; ++j) {
          const float cx = xyz[3 * j], cy = xyz[3 * j + 1], cz = xyz[3 * j + 2];
          if (gn::finite3(cx, cy, cz)) gn::visit(mo, cx - qx, cy - qy, cz - qz, t);
        }
      gn::store(mo, out_moments + i * gn::kMomentWords);
    }
  };
  const int64_t workers = std::max<int64_t>(1, std::min<int64_t>({8, static_cast<int64_t>(std::thread::hardware_concurrency()), n / 1024}));
  std::vector<std::thread> pool;
  for (int64_t w = 1; w < workers; ++w) pool.emplace_back(rows, n * w / workers, n * (w + 1) / workers);
  rows(0, n / workers);
  for (std::thread &th : pool) th.join();
  return PCP_OK;
}

int pcp_frame_geometry(pcp_context *ctx, int32_t frame, int32_t *out_index, float *out_range, float *out_xyz_cam,
                       float *out_normal_cam, int64_t *out_pixels) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_pixels) *out_pixels = 0;
  if (out_normal_cam && !ctx->gn_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_frame_geometry: normal_cam needs pcp_estimate_normals on this cloud");
  int rc = frame_geometry_device(ctx, "pcp_frame_geometry", frame, out_normal_cam != nullptr);
  if (rc != PCP_OK) return rc;
  const int64_t px = static_cast<int64_t>(ctx->dcam.img_w) * ctx->dcam.img_h;
  if (px <= 0) return PCP_OK;
  const size_t spx = static_cast<size_t>(px);
  const int32_t *d_index = reinterpret_cast<const int32_t *>(ctx->gm_out.p);
  const float *d_range = reinterpret_cast<const float *>(ctx->gm_out.p + spx);
  const float *d_xyz = reinterpret_cast<const float *>(ctx->gm_out.p + 2 * spx);
  const float *d_normal = reinterpret_cast<const float *>(ctx->gm_out.p + 5 * spx);
  unsigned long long occupied = 0;
  PCP_HIP_TRY(ctx, hipMemcpyAsync(&occupied, ctx->s_counter.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out_index) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_index, d_index, spx * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_range) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_range, d_range, spx * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_xyz_cam) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_xyz_cam, d_xyz, 3 * spx * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_normal_cam) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_normal_cam, d_normal, 3 * spx * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (out_pixels) *out_pixels = static_cast<int64_t>(occupied);
  return PCP_OK;
}

}  // extern "C"
