// pcp_crack_width.hip -- crack width maps ("Crack width maps", CW1-CW9): for every foreground pixel of a
// keyframe's mask the two edge points along the exact EDT direction, the plane of the position image's window around the
// pixel, and the 3-D distance between the two edge rays' intersections with that plane -- what compute_skeleton_edge_pts of
// scripts/genNormAndDistanceMask.py (:396-478; find_edges_by_direction / trace_edge :706-762, find_local_plane :601-636,
// search_3d_edge_points :564-599) does on the host, with the grid search replaced by the intersection it approximates.
//
// The call runs the keyframe's distance transform (pcp_mask_edt.hip) and geometry scatter (pcp_normals.hip) on the device
// and reads their results where they lie.  The position image is sparse and the plane is needed at every site, so the
// window sums come from summed-area tables of the ten origin moments of the quantised positions: one kernel quantises, a
// row scan and a segmented column scan take the prefix sums modulo 2^64, and the site kernel reads four corners per moment
// and recentres them (pcp_crack_width.hpp), which is exact because the recentred values fit 64 bits.  No atomics but the
// two counts, one per wavefront; every loop is bounded by the image size.
#include <algorithm>
#include <new>
#include <thread>
#include <vector>

#include "pcp_internal.hpp"
#include "pcp_crack_map.hpp"
#include "pcp_eigen33.hpp"
#include "pcp_crack_width.hpp"

namespace pcp {

constexpr int kCwBlock = 256;
constexpr int kCwRowTile = 4 * kCwBlock;  // row scan: four consecutive pixels per lane and round
constexpr int32_t kCwSegmentRows = 64;    // column scan: rows per segment

static inline uint32_t cw_blocks(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kCwBlock))); }

// ---- the origin moments of the members (CW4), one lane per pixel ----------------------------------------------------------
__global__ __launch_bounds__(kCwBlock) void k_cw_quantise(const int32_t *__restrict__ index, const float *__restrict__ xyz,
                                                          int64_t px, unsigned long long *__restrict__ sat) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kCwBlock + threadIdx.x;
  if (p >= px) return;
  uint64_t t[cw::kOriginPlanes];
#pragma unroll
  for (int a = 0; a < cw::kOriginPlanes; ++a) t[a] = 0;
  if (index[p] >= 0) {
    const float x = xyz[3 * p + 0], y = xyz[3 * p + 1], z = xyz[3 * p + 2];
    if (cw::member_ok(x, y, z)) cw::origin_terms(cw::quantise(x), cw::quantise(y), cw::quantise(z), t);
  }
#pragma unroll
  for (int a = 0; a < cw::kOriginPlanes; ++a) sat[a * px + p] = t[a];
}

// ---- row scan: one workgroup per (row, plane); the wavefronts' sums meet in LDS, the carry runs along the row ----------------
__global__ __launch_bounds__(kCwBlock) void k_cw_rows(unsigned long long *__restrict__ sat, int32_t w, int32_t h) {
  __shared__ unsigned long long ws[kCwBlock / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned long long *row = sat + (static_cast<int64_t>(blockIdx.y) * h + static_cast<int64_t>(blockIdx.x)) * w;
  unsigned long long carry = 0;
  for (int32_t base = 0; base < w; base += kCwRowTile) {
    const int32_t i0 = base + static_cast<int32_t>(threadIdx.x) * 4;
    unsigned long long v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < w ? row[i0 + k] : 0ull;
#pragma unroll
    for (int k = 1; k < 4; ++k) v[k] += v[k - 1];
    const unsigned long long mine = v[3];
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) ws[wid] = incl;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kCwBlock / 64; ++k) {
      if (k < wid) before += ws[k];
      total += ws[k];
    }
    __syncthreads();  // (ws is written again in the next round)
    const unsigned long long off = carry + before + (incl - mine);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < w) row[i0 + k] = off + v[k];
    carry += total;
  }
}

// ---- column scan, segmented as k_md_columns is: one lane per (column, segment of 64 rows, plane) ---------------------------
__global__ __launch_bounds__(kCwBlock) void k_cw_column_sums(const unsigned long long *__restrict__ sat, int32_t w, int32_t h,
                                                             int32_t segs, unsigned long long *__restrict__ seg) {
  const int32_t x = static_cast<int32_t>(blockIdx.x) * kCwBlock + static_cast<int32_t>(threadIdx.x);
  if (x >= w) return;
  const int32_t s = static_cast<int32_t>(blockIdx.y), a = static_cast<int32_t>(blockIdx.z);
  const unsigned long long *col = sat + static_cast<int64_t>(a) * h * w + x;
  const int32_t y0 = s * kCwSegmentRows, y1 = min(h, y0 + kCwSegmentRows);
  unsigned long long sum = 0;
  for (int32_t y = y0; y < y1; ++y) sum += col[static_cast<int64_t>(y) * w];
  seg[(static_cast<int64_t>(a) * segs + s) * w + x] = sum;
}

__global__ __launch_bounds__(kCwBlock) void k_cw_columns(unsigned long long *__restrict__ sat, int32_t w, int32_t h, int32_t segs,
                                                         const unsigned long long *__restrict__ seg) {
  const int32_t x = static_cast<int32_t>(blockIdx.x) * kCwBlock + static_cast<int32_t>(threadIdx.x);
  if (x >= w) return;
  const int32_t s = static_cast<int32_t>(blockIdx.y), a = static_cast<int32_t>(blockIdx.z);
  const unsigned long long *sg = seg + static_cast<int64_t>(a) * segs * w + x;
  unsigned long long run = 0;
  for (int32_t sp = 0; sp < s; ++sp) run += sg[static_cast<int64_t>(sp) * w];
  unsigned long long *col = sat + static_cast<int64_t>(a) * h * w + x;
  const int32_t y0 = s * kCwSegmentRows, y1 = min(h, y0 + kCwSegmentRows);
  for (int32_t y = y0; y < y1; ++y) {
    run += col[static_cast<int64_t>(y) * w];
    col[static_cast<int64_t>(y) * w] = run;
  }
}

// ---- the sites -------------------------------------------------------------------------------------------------------------
struct CwSiteArgs {
  int32_t w, h, radius;
  const unsigned long long *bits;  // md_bits of the keyframe: bit (y & 63) of word (y >> 6) * w + x = background
  const uint32_t *d2;
  const int32_t *nearest;
  const unsigned long long *sat;  // ten planes of w * h
  cw::Intrinsics cam;
  // outputs, each nullable
  uint8_t *flags;
  int32_t *edges;
  uint32_t *w2d2;
  float *width, *points, *plane;
  long long *moments;
  unsigned long long *tally;  // [0] += sites, [1] += widths
};

// one lane per pixel: x along the workgroup, y = blockIdx.y
__global__ __launch_bounds__(kCwBlock) void k_cw_sites(CwSiteArgs g) {
  const int32_t x = static_cast<int32_t>(blockIdx.x) * kCwBlock + static_cast<int32_t>(threadIdx.x);
  const int32_t y = static_cast<int32_t>(blockIdx.y);
  const int32_t w = g.w, h = g.h;
  const bool inside = x < w;
  const int64_t p = static_cast<int64_t>(y) * w + (inside ? x : 0);
  auto bg = [&](int32_t qx, int32_t qy) -> bool { return (g.bits[static_cast<int64_t>(qy >> 6) * w + qx] >> (qy & 63)) & 1ull; };
  uint32_t flags = 0, w2 = 0;
  cw::Edge near_e{0, -1, -1}, far_e{0, -1, -1};
  int64_t mom[cw::kMomentWords];
#pragma unroll
  for (int a = 0; a < cw::kMomentWords; ++a) mom[a] = 0;
  float pl[4] = {0.0f, 0.0f, 0.0f, 0.0f}, pts[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, width = 0.0f;
  if (inside && !bg(x, y)) {
    flags = cw::kSite;
    {  // CW4 / CW5: four corners per origin moment
      int32_t x0, x1, y0, y1;
      cw::window(x, g.radius, w, x0, x1);
      cw::window(y, g.radius, h, y0, y1);
      const int64_t px = static_cast<int64_t>(w) * h;
      uint64_t o[cw::kOriginPlanes];
#pragma unroll
      for (int a = 0; a < cw::kOriginPlanes; ++a) {
        const unsigned long long *pa = g.sat + a * px;
        o[a] = cw::window_sum([&](int32_t qx, int32_t qy) -> uint64_t { return pa[static_cast<int64_t>(qy) * w + qx]; }, x0, x1, y0, y1);
      }
      cw::recentre(o, mom);
    }
    const uint32_t d2 = g.d2[p];
    if (d2 != cw::kSentinelD2) {  // CW1: a mask without background has sites and nothing else
      if (cw::is_centre([&](int32_t qx, int32_t qy) -> uint32_t { return g.d2[static_cast<int64_t>(qy) * w + qx]; }, x, y, w, h))
        flags |= cw::kCentre;
      const int32_t e1 = g.nearest[p];
      const int32_t ey = e1 / w, ex = e1 - ey * w;
      near_e = cw::trace(bg, x, y, x - ex, y - ey, -1, w, h);
      far_e = cw::trace(bg, x, y, x - ex, y - ey, +1, w, h);
      if (near_e.found) flags |= cw::kNear;
      if (far_e.found) flags |= cw::kFar;
      if (near_e.found && far_e.found) w2 = cw::edge_distance2(near_e, far_e);
      if (mom[0] >= cw::kMinMembers) {  // CW6
        double C[6], ev, n[3], c[3];
        cw::covariance(mom, C);
        smallest_eigenpair(C, ev, n);
        const float nx = static_cast<float>(n[0]), ny = static_cast<float>(n[1]), nz = static_cast<float>(n[2]);
        if (fabsf(nx) <= 3.402823466e+38f && fabsf(ny) <= 3.402823466e+38f && fabsf(nz) <= 3.402823466e+38f) {
          flags |= cw::kPlane;
          cw::centroid(mom, c);
          const double nc = cw::orient(n, c);
          pl[0] = static_cast<float>(n[0]);
          pl[1] = static_cast<float>(n[1]);
          pl[2] = static_cast<float>(n[2]);
          pl[3] = static_cast<float>(-nc);
          if (near_e.found && far_e.found) {  // CW7 / CW8
            double a[3], b[3];
            const bool ok = cw::edge_point(g.cam, n, nc, near_e.ex, near_e.ey, a) & cw::edge_point(g.cam, n, nc, far_e.ex, far_e.ey, b);
            if (ok) {
              flags |= cw::kRays | cw::kWidth;
              width = static_cast<float>(cw::width_of(a, b));
#pragma unroll
              for (int k = 0; k < 3; ++k) {
                pts[k] = static_cast<float>(a[k]);
                pts[3 + k] = static_cast<float>(b[k]);
              }
            }
          }
        }
      }
    }
  }
  const unsigned long long sites = __ballot(flags & cw::kSite), widths = __ballot(flags & cw::kWidth);
  if ((threadIdx.x & 63) == 0) {
    if (sites) atomicAdd(g.tally, static_cast<unsigned long long>(__popcll(sites)));
    if (widths) atomicAdd(g.tally + 1, static_cast<unsigned long long>(__popcll(widths)));
  }
  if (!inside) return;
  if (g.flags) g.flags[p] = static_cast<uint8_t>(flags);
  if (g.edges) reinterpret_cast<int4 *>(g.edges)[p] = make_int4(near_e.ex, near_e.ey, far_e.ex, far_e.ey);
  if (g.w2d2) g.w2d2[p] = w2;
  if (g.width) g.width[p] = width;
  if (g.points) {
#pragma unroll
    for (int k = 0; k < 6; ++k) g.points[6 * p + k] = pts[k];
  }
  if (g.plane) reinterpret_cast<float4 *>(g.plane)[p] = make_float4(pl[0], pl[1], pl[2], pl[3]);
  if (g.moments) {
#pragma unroll
    for (int a = 0; a < cw::kMomentWords; ++a) g.moments[cw::kMomentWords * p + a] = mom[a];
  }
}

hipError_t preload_crack_width() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_cw_sites));
}

static cw::Intrinsics intrinsics_of(const DevCamera &c) { return cw::Intrinsics{c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3}; }

// The call's own kernels, after the two stages have left their maps on the device: the device part, for the callers that read
// the results where they lie (pcp_crack_fuse.hip).  The wanted outputs stay in ctx->cw_flags, cw_i32 (edges | w2d2), cw_f32
// (plane | width | points) and cw_moments, the two counts in ctx->s_counter[2..3]; nothing is copied, no synchronisation.
int crack_width_device(pcp_context *ctx, const pcp_crack_params &prm, const CrackWidthWant &want) {
  const bool out_flags = want.flags, out_edges = want.edges, out_w2d2 = want.w2d2, out_width = want.width, out_points = want.points,
             out_plane = want.plane, out_moments = want.moments;
  const int32_t w = ctx->dcam.img_w, h = ctx->dcam.img_h;
  const int64_t px = static_cast<int64_t>(w) * h;
  const size_t spx = static_cast<size_t>(px);
  const int32_t segs = (h + kCwSegmentRows - 1) / kCwSegmentRows;
  const size_t planes = static_cast<size_t>(cw::kOriginPlanes) * spx;
  PCP_HIP_TRY(ctx, ctx->cw_sat.ensure(planes + static_cast<size_t>(cw::kOriginPlanes) * segs * w + 4));
  if (out_flags) PCP_HIP_TRY(ctx, ctx->cw_flags.ensure(spx + 16));
  if (out_edges || out_w2d2) PCP_HIP_TRY(ctx, ctx->cw_i32.ensure(5 * spx + 4));
  if (out_width || out_points || out_plane) PCP_HIP_TRY(ctx, ctx->cw_f32.ensure(11 * spx + 4));
  if (out_moments) PCP_HIP_TRY(ctx, ctx->cw_moments.ensure(static_cast<size_t>(cw::kMomentWords) * spx + 4));
  PCP_HIP_TRY(ctx, ctx->s_counter.ensure(4));
  unsigned long long *tally = ctx->s_counter.p + 2;  // (word 0 is the geometry scatter's occupied count)
  PCP_HIP_TRY(ctx, hipMemsetAsync(tally, 0, 16, ctx->stream));
  unsigned long long *seg = ctx->cw_sat.p + planes;
  CwSiteArgs g{};
  g.w = w;
  g.h = h;
  g.radius = prm.plane_radius_px;
  g.bits = ctx->md_bits.p;
  g.d2 = ctx->md_d2.p;
  g.nearest = ctx->md_nearest.p;
  g.sat = ctx->cw_sat.p;
  g.cam = intrinsics_of(ctx->dcam);
  g.flags = out_flags ? ctx->cw_flags.p : nullptr;
  g.edges = out_edges ? ctx->cw_i32.p : nullptr;
  g.w2d2 = out_w2d2 ? reinterpret_cast<uint32_t *>(ctx->cw_i32.p + 4 * spx) : nullptr;
  g.plane = out_plane ? ctx->cw_f32.p : nullptr;  // (first: written as float4)
  g.width = out_width ? ctx->cw_f32.p + 4 * spx : nullptr;
  g.points = out_points ? ctx->cw_f32.p + 5 * spx : nullptr;
  g.moments = out_moments ? ctx->cw_moments.p : nullptr;
  g.tally = tally;
  const uint32_t xb = static_cast<uint32_t>((w + kCwBlock - 1) / kCwBlock);
  {
    LaunchTimer lt(ctx, PCP_K_MISC);  // the summed-area tables
    hipLaunchKernelGGL(k_cw_quantise, dim3(cw_blocks(px)), dim3(kCwBlock), 0, ctx->stream, reinterpret_cast<const int32_t *>(ctx->gm_out.p),
                       reinterpret_cast<const float *>(ctx->gm_out.p + 2 * spx), px, ctx->cw_sat.p);
    hipLaunchKernelGGL(k_cw_rows, dim3(static_cast<uint32_t>(h), cw::kOriginPlanes), dim3(kCwBlock), 0, ctx->stream, ctx->cw_sat.p, w, h);
    hipLaunchKernelGGL(k_cw_column_sums, dim3(xb, static_cast<uint32_t>(segs), cw::kOriginPlanes), dim3(kCwBlock), 0, ctx->stream,
                       ctx->cw_sat.p, w, h, segs, seg);
    hipLaunchKernelGGL(k_cw_columns, dim3(xb, static_cast<uint32_t>(segs), cw::kOriginPlanes), dim3(kCwBlock), 0, ctx->stream, ctx->cw_sat.p,
                       w, h, segs, seg);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer lt(ctx, PCP_K_MISC);  // the sites
    hipLaunchKernelGGL(k_cw_sites, dim3(xb, static_cast<uint32_t>(h)), dim3(kCwBlock), 0, ctx->stream, g);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return PCP_OK;
}

// ... and with the downloads of pcp_crack_width
static int crack_width_run(pcp_context *ctx, const pcp_crack_params &prm, uint8_t *out_flags, int32_t *out_edges, uint32_t *out_w2d2,
                           float *out_width, float *out_points, float *out_plane, int64_t *out_moments, int64_t *out_sites,
                           int64_t *out_widths) {
  const CrackWidthWant want{out_flags != nullptr, out_edges != nullptr,  out_w2d2 != nullptr,   out_width != nullptr,
                            out_points != nullptr, out_plane != nullptr, out_moments != nullptr};
  const int rc = crack_width_device(ctx, prm, want);
  if (rc != PCP_OK) return rc;
  const size_t spx = static_cast<size_t>(ctx->dcam.img_w) * static_cast<size_t>(ctx->dcam.img_h);
  const unsigned long long *tally = ctx->s_counter.p + 2;
  unsigned long long counts[2] = {0, 0};
  PCP_HIP_TRY(ctx, hipMemcpyAsync(counts, tally, 16, hipMemcpyDeviceToHost, ctx->stream));
  if (out_flags) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_flags, ctx->cw_flags.p, spx, hipMemcpyDeviceToHost, ctx->stream));
  if (out_edges) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_edges, ctx->cw_i32.p, 4 * spx * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_w2d2) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_w2d2, ctx->cw_i32.p + 4 * spx, spx * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_width) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_width, ctx->cw_f32.p + 4 * spx, spx * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_points) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_points, ctx->cw_f32.p + 5 * spx, 6 * spx * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_plane) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_plane, ctx->cw_f32.p, 4 * spx * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_moments)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_moments, ctx->cw_moments.p, static_cast<size_t>(cw::kMomentWords) * spx * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (out_sites) *out_sites = static_cast<int64_t>(counts[0]);
  if (out_widths) *out_widths = static_cast<int64_t>(counts[1]);
  return PCP_OK;
}

// the checks of the arguments pcp_crack_width and pcp_crack_fuse_add share, under the caller's name
int crack_width_check(pcp_context *ctx, const char *who, const pcp_crack_params *params) {
  if (!params) return set_error(ctx, PCP_ERR_INVALID, "%s: params is NULL", who);
  if (params->threshold < 0 || params->threshold > 255)
    return set_error(ctx, PCP_ERR_INVALID, "%s: threshold %d outside 0..255", who, params->threshold);
  if (!cw::radius_ok(params->plane_radius_px))
    return set_error(ctx, PCP_ERR_INVALID, "%s: plane_radius_px %d outside %d..%d", who, params->plane_radius_px, cw::kMinRadius,
                     cw::kMaxRadius);
  if (ctx->have_camera) {
    const int64_t w = ctx->dcam.img_w, h = ctx->dcam.img_h;
    if (w > cw::kMaxSide || h > cw::kMaxSide || w * h > cw::kMaxPixels)
      return set_error(ctx, PCP_ERR_RANGE, "%s: image %d x %d exceeds %d a side or 2^26 pixels", who, static_cast<int>(w),
                       static_cast<int>(h), cw::kMaxSide);
  }
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_crack_width(pcp_context *ctx, int32_t frame, const pcp_crack_params *params, uint8_t *out_flags, int32_t *out_edges,
                    uint32_t *out_w2d2, float *out_width, float *out_points, float *out_plane, int64_t *out_moments,
                    int64_t *out_sites, int64_t *out_widths) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_sites) *out_sites = 0;
  if (out_widths) *out_widths = 0;
  int rc = crack_width_check(ctx, "pcp_crack_width", params);
  if (rc != PCP_OK) return rc;
  // the geometry scatter first (camera, cloud, keyframes, the keyframe's range), then the distance transform (the mask)
  if ((rc = frame_geometry_device(ctx, "pcp_crack_width", frame, /*with_normals=*/false)) != PCP_OK) return rc;
  if (ctx->dcam.img_w <= 0 || ctx->dcam.img_h <= 0) return PCP_OK;
  if ((rc = mask_edt_device(ctx, "pcp_crack_width", frame, params->threshold)) != PCP_OK) return rc;
  return crack_width_run(ctx, *params, out_flags, out_edges, out_w2d2, out_width, out_points, out_plane, out_moments, out_sites, out_widths);
}

int pcp_crack_width_host(int32_t width, int32_t height, const uint8_t *gray, int64_t row_stride_bytes, const int32_t *index_image,
                         const float *xyz_cam_image, const pcp_crack_params *params, uint8_t *out_flags, int32_t *out_edges,
                         uint32_t *out_w2d2, int64_t *out_moments) {
  if (width <= 0 || height <= 0 || !gray || !index_image || !xyz_cam_image || row_stride_bytes < static_cast<int64_t>(width)) {
    set_global_error("pcp_crack_width_host: empty image, NULL mask, index or position image, or row stride < width");
    return PCP_ERR_INVALID;
  }
  if (!params || params->threshold < 0 || params->threshold > 255 || !cw::radius_ok(params->plane_radius_px)) {
    set_global_error("pcp_crack_width_host: NULL params, threshold outside 0..255 or plane_radius_px outside %d..%d", cw::kMinRadius,
                     cw::kMaxRadius);
    return PCP_ERR_INVALID;
  }
  if (width > cw::kMaxSide || height > cw::kMaxSide || static_cast<int64_t>(width) * height > cw::kMaxPixels) {
    set_global_error("pcp_crack_width_host: image %d x %d exceeds %d a side or 2^26 pixels", width, height, cw::kMaxSide);
    return PCP_ERR_RANGE;
  }
  const int32_t w = width, h = height, radius = params->plane_radius_px;
  const size_t px = static_cast<size_t>(w) * static_cast<size_t>(h);
  std::vector<uint32_t> d2;
  std::vector<int32_t> nearest;
  std::vector<uint64_t> sat;
  try {
    d2.resize(px);
    nearest.resize(px);
    sat.assign(static_cast<size_t>(cw::kOriginPlanes) * px, 0);
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_crack_width_host: out of host memory for %d x %d pixels", width, height);
    return PCP_ERR_NOMEM;
  }
  const int rc = pcp_mask_edt_host(width, height, gray, row_stride_bytes, params->threshold, d2.data(), nearest.data());
  if (rc != PCP_OK) return rc;
  // the summed-area tables, modulo 2^64: members, then along the rows, then down the columns
  for (size_t p = 0; p < px; ++p) {
    if (index_image[p] < 0) continue;
    const float x = xyz_cam_image[3 * p], y = xyz_cam_image[3 * p + 1], z = xyz_cam_image[3 * p + 2];
    if (!cw::member_ok(x, y, z)) continue;
    uint64_t t[cw::kOriginPlanes];
    cw::origin_terms(cw::quantise(x), cw::quantise(y), cw::quantise(z), t);
    for (int a = 0; a < cw::kOriginPlanes; ++a) sat[static_cast<size_t>(a) * px + p] = t[a];
  }
  for (int a = 0; a < cw::kOriginPlanes; ++a) {
    uint64_t *pa = sat.data() + static_cast<size_t>(a) * px;
    for (int32_t y = 0; y < h; ++y) {
      uint64_t *row = pa + static_cast<size_t>(y) * w;
      for (int32_t x = 1; x < w; ++x) row[x] += row[x - 1];
      if (y > 0)
        for (int32_t x = 0; x < w; ++x) row[x] += row[x - w];
    }
  }
  auto bg = [&](int32_t qx, int32_t qy) -> bool {
    return !(static_cast<int32_t>(gray[static_cast<int64_t>(qy) * row_stride_bytes + qx]) > params->threshold);
  };
  auto d2_at = [&](int32_t qx, int32_t qy) -> uint32_t { return d2[static_cast<size_t>(qy) * w + qx]; };
  // the sites: the rows do not interact, up to 8 host threads share them
  auto rows = [&](int32_t r0, int32_t r1) {
    for (int32_t y = r0; y < r1; ++y)
      for (int32_t x = 0; x < w; ++x) {
        const size_t p = static_cast<size_t>(y) * w + x;
        uint32_t flags = 0, w2 = 0;
        cw::Edge near_e{0, -1, -1}, far_e{0, -1, -1};
        int64_t mom[cw::kMomentWords] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (!bg(x, y)) {
          flags = cw::kSite;
          if (out_moments) {
            int32_t x0, x1, y0, y1;
            cw::window(x, radius, w, x0, x1);
            cw::window(y, radius, h, y0, y1);
            uint64_t o[cw::kOriginPlanes];
            for (int a = 0; a < cw::kOriginPlanes; ++a) {
              const uint64_t *pa = sat.data() + static_cast<size_t>(a) * px;
              o[a] = cw::window_sum([&](int32_t qx, int32_t qy) -> uint64_t { return pa[static_cast<size_t>(qy) * w + qx]; }, x0, x1, y0, y1);
            }
            cw::recentre(o, mom);
          }
          if (d2[p] != cw::kSentinelD2) {
            if (cw::is_centre(d2_at, x, y, w, h)) flags |= cw::kCentre;
            const int32_t e1 = nearest[p];
            const int32_t ey = e1 / w, ex = e1 - ey * w;
            near_e = cw::trace(bg, x, y, x - ex, y - ey, -1, w, h);
            far_e = cw::trace(bg, x, y, x - ex, y - ey, +1, w, h);
            if (near_e.found) flags |= cw::kNear;
            if (far_e.found) flags |= cw::kFar;
            if (near_e.found && far_e.found) w2 = cw::edge_distance2(near_e, far_e);
          }
        }
        if (out_flags) out_flags[p] = static_cast<uint8_t>(flags);
        if (out_edges) {
          out_edges[4 * p + 0] = near_e.ex;
          out_edges[4 * p + 1] = near_e.ey;
          out_edges[4 * p + 2] = far_e.ex;
          out_edges[4 * p + 3] = far_e.ey;
        }
        if (out_w2d2) out_w2d2[p] = w2;
        if (out_moments)
          for (int a = 0; a < cw::kMomentWords; ++a) out_moments[static_cast<size_t>(cw::kMomentWords) * p + a] = mom[a];
      }
  };
  const int32_t workers = static_cast<int32_t>(
      std::max<int64_t>(1, std::min<int64_t>({8, static_cast<int64_t>(std::thread::hardware_concurrency()), height / 64})));
  std::vector<std::thread> pool;
  for (int32_t k = 1; k < workers; ++k)
    pool.emplace_back(rows, static_cast<int32_t>(static_cast<int64_t>(height) * k / workers),
                      static_cast<int32_t>(static_cast<int64_t>(height) * (k + 1) / workers));
  rows(0, height / workers);
  for (std::thread &th : pool) th.join();
  return PCP_OK;
}

}  // extern "C"
