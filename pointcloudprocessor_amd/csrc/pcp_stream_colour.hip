// pcp_stream_colour.hip -- the pieces that let a cloud larger than one upload be coloured chunk by chunk (DESIGN.md,
// "Streamed colourisation"): the depth-map accumulator that outlives the uploads (a chunk of a streamed cloud is an index
// shard in time: the maps are a MIN over all points), and removePointsWithNoColor on the device.
#include <algorithm>

#include "pcp_internal.hpp"

namespace pcp {

constexpr int kScBlock = 256;
constexpr uint32_t kFarBits = 0x7f7fffffu;  // FLT_MAX: the "far" value of the depth maps (view_culling.cpp:64)

__global__ __launch_bounds__(kScBlock) void k_sc_fill(uint32_t *__restrict__ p, int64_t n, uint32_t v) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * kScBlock + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kScBlock;
  for (; i < n; i += stride) p[i] = v;
}

// acc = min(acc, maps) over the bit patterns: the maps hold positive floats (ranges, or FLT_MAX), whose order is the order
// of their bits as unsigned integers.  Four cells per lane (both buffers come from hipMalloc: 16-byte aligned), a scalar tail.
__global__ __launch_bounds__(kScBlock) void k_depth_accum_min(uint32_t *__restrict__ acc, const uint32_t *__restrict__ maps,
                                                             int64_t n) {
  const int64_t quads = n >> 2;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kScBlock;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kScBlock + threadIdx.x;
  uint4 *a4 = reinterpret_cast<uint4 *>(acc);
  const uint4 *m4 = reinterpret_cast<const uint4 *>(maps);
  for (int64_t q = t; q < quads; q += stride) {
    uint4 a = a4[q];
    const uint4 m = m4[q];
    a.x = min(a.x, m.x);
    a.y = min(a.y, m.y);
    a.z = min(a.z, m.z);
    a.w = min(a.w, m.w);
    a4[q] = a;
  }
  const int64_t i = (quads << 2) + t;
  if (i < n) acc[i] = min(acc[i], maps[i]);
}

// the has byte of every packed colour word, as the flags compact_flags takes
__global__ __launch_bounds__(kScBlock) void k_has_flags(const uint32_t *__restrict__ packed, int64_t n, uint8_t *__restrict__ flag) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kScBlock + threadIdx.x;
  if (i < n) flag[i] = (packed[i] >> 24) ? uint8_t(1) : uint8_t(0);
}

// row k of the compacted result = point index[k] of the uploaded cloud: its coordinates bit for bit, r g b, the fused label
__global__ __launch_bounds__(kScBlock) void k_compact_gather(const int32_t *__restrict__ index, int64_t m,
                                                            const float *__restrict__ x, const float *__restrict__ y,
                                                            const float *__restrict__ z, const uint32_t *__restrict__ packed,
                                                            const uint32_t *__restrict__ labels, float *__restrict__ out_xyz,
                                                            uint8_t *__restrict__ out_rgb, uint8_t *__restrict__ out_label) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kScBlock + threadIdx.x;
  if (k >= m) return;
  const int32_t i = index[k];
  if (out_xyz) {
    out_xyz[3 * k + 0] = x[i];
    out_xyz[3 * k + 1] = y[i];
    out_xyz[3 * k + 2] = z[i];
  }
  if (out_rgb) {
    const uint32_t v = packed[i];
    out_rgb[3 * k + 0] = static_cast<uint8_t>(v & 0xffu);
    out_rgb[3 * k + 1] = static_cast<uint8_t>((v >> 8) & 0xffu);
    out_rgb[3 * k + 2] = static_cast<uint8_t>((v >> 16) & 0xffu);
  }
  if (out_label) out_label[k] = static_cast<uint8_t>(labels[i] & 0xffu);
}

hipError_t preload_stream_colour() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_depth_accum_min));
}

static inline int64_t map_floats(const pcp_context *ctx) {
  return static_cast<int64_t>(ctx->dcam.mw) * ctx->dcam.mh * ctx->n_frames;
}
static inline uint32_t sc_blocks(int64_t n, int64_t cap) {
  return static_cast<uint32_t>(std::max<int64_t>(1, std::min<int64_t>(div_up(n, kScBlock), cap)));
}

// what all four accumulator calls need: camera and keyframes, not PCP_CULL_HPR; the accumulator itself unless `reset`
static int accum_ready(pcp_context *ctx, const char *who, bool reset) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!ctx->have_camera) return set_error(ctx, PCP_ERR_STATE, "%s: pcp_set_camera has not been called", who);
  if (ctx->n_frames <= 0) return set_error(ctx, PCP_ERR_STATE, "%s: pcp_set_frames has not been called", who);
  if (ctx->cull.cull_mode == PCP_CULL_HPR)
    return set_error(ctx, PCP_ERR_STATE, "%s: PCP_CULL_HPR has no depth maps to merge across parts of a cloud (the hull needs the "
                     "whole map at once)", who);
  if (!reset && (!ctx->depth_accum_live || !ctx->depth_accum.p))
    return set_error(ctx, PCP_ERR_STATE, "%s: no accumulator (call pcp_depth_accum_reset; pcp_set_camera and pcp_set_frames drop it)", who);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return set_error(ctx, PCP_ERR_DEVICE, "%s: hipSetDevice failed: %s", who, hipGetErrorString(e));
  return PCP_OK;
}

// merge and apply work on the maps of the cloud that is uploaded now
static int maps_current(pcp_context *ctx, const char *who) {
  for (int32_t f = 0; f < ctx->n_frames; ++f)
    if (!ctx->depth.p || static_cast<size_t>(f) >= ctx->depth_valid.size() || !ctx->depth_valid[static_cast<size_t>(f)])
      return set_error(ctx, PCP_ERR_STATE, "%s: pcp_depth_pass has not covered keyframe %d since the latest upload", who, f);
  return PCP_OK;
}

int colour_compact_indices(pcp_context *ctx, int64_t *m) {
  const int64_t n = ctx->n;
  const size_t sn = static_cast<size_t>(n);
  const uint32_t *packed = ctx->rgba2[ctx->rgba_cur].p;
  PCP_HIP_TRY(ctx, ctx->s_keep.ensure(4 * sn + 16));
  PCP_HIP_TRY(ctx, ctx->s_cell.ensure(sn + 4));
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_has_flags, dim3(sc_blocks(n, int64_t(1) << 31)), dim3(kScBlock), 0, ctx->stream, packed, n, ctx->s_keep.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return compact_flags(ctx, ctx->s_keep.p, n, ctx->s_cell.p, n, m);
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_depth_accum_reset(pcp_context *ctx) {
  int rc = accum_ready(ctx, "pcp_depth_accum_reset", true);
  if (rc != PCP_OK) return rc;
  const int64_t n = map_floats(ctx);
  ctx->depth_accum_live = false;
  PCP_HIP_TRY(ctx, ctx->depth_accum.ensure(static_cast<size_t>(n) + 4));
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_sc_fill, dim3(sc_blocks(n, 8192)), dim3(kScBlock), 0, ctx->stream, ctx->depth_accum.p, n, kFarBits);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  ctx->depth_accum_live = true;
  return PCP_OK;
}

int pcp_depth_accum_merge(pcp_context *ctx) {
  int rc = accum_ready(ctx, "pcp_depth_accum_merge", false);
  if (rc != PCP_OK) return rc;
  if ((rc = maps_current(ctx, "pcp_depth_accum_merge")) != PCP_OK) return rc;
  const int64_t n = map_floats(ctx);
  LaunchTimer t(ctx, PCP_K_MISC);
  hipLaunchKernelGGL(k_depth_accum_min, dim3(sc_blocks(div_up(n, 4), 4096)), dim3(kScBlock), 0, ctx->stream, ctx->depth_accum.p,
                     ctx->depth.p, n);
  PCP_HIP_TRY(ctx, hipGetLastError());
  return PCP_OK;
}

int pcp_depth_accum_apply(pcp_context *ctx) {
  int rc = accum_ready(ctx, "pcp_depth_accum_apply", false);
  if (rc != PCP_OK) return rc;
  if ((rc = maps_current(ctx, "pcp_depth_accum_apply")) != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, hipMemcpyAsync(ctx->depth.p, ctx->depth_accum.p, static_cast<size_t>(map_floats(ctx)) * 4, hipMemcpyDeviceToDevice,
                                  ctx->stream));
  return PCP_OK;
}

int pcp_depth_accum_device(pcp_context *ctx, void **device_ptr, int64_t *n_floats) {
  int rc = accum_ready(ctx, "pcp_depth_accum_device", false);
  if (rc != PCP_OK) return rc;
  if (device_ptr) *device_ptr = ctx->depth_accum.p;
  if (n_floats) *n_floats = map_floats(ctx);
  return PCP_OK;
}

int pcp_colour_compact(pcp_context *ctx, int64_t capacity, int32_t *out_index, float *out_xyz, uint8_t *out_rgb, uint8_t *out_label,
                       int64_t *out_count) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_count) *out_count = 0;
  if (capacity < 0) return set_error(ctx, PCP_ERR_INVALID, "pcp_colour_compact: negative capacity");
  if (!ctx->colour_result_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_colour_compact: no result (call pcp_colorize / pcp_colorize_from_depth / pcp_colour_finalise)");
  if (out_label && !ctx->labels_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_colour_compact: out_label asked of a result made without label fusion (pcp_set_label_fusion)");
  const int64_t n = ctx->n;
  if (n == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sn = static_cast<size_t>(n);
  const uint32_t *packed = ctx->rgba2[ctx->rgba_cur].p;
  int64_t m = 0;
  int rc = colour_compact_indices(ctx, &m);
  if (rc != PCP_OK) return rc;
  if (out_count) *out_count = m;
  const int64_t take = std::min(m, capacity);
  if (take == 0 || !(out_index || out_xyz || out_rgb || out_label)) return PCP_OK;
  const size_t st = static_cast<size_t>(take);
  if (out_xyz || out_rgb || out_label) {
    // xyz (12 B) | rgb (3 B) | label (1 B) per row, each section from a 16-byte boundary
    const size_t rgb_off = (12 * st + 15) & ~size_t(15), label_off = (rgb_off + 3 * st + 15) & ~size_t(15);
    PCP_HIP_TRY(ctx, ctx->cc_out.ensure(label_off + st + 16));
    float *d_xyz = reinterpret_cast<float *>(ctx->cc_out.p);
    uint8_t *d_rgb = ctx->cc_out.p + rgb_off, *d_label = ctx->cc_out.p + label_off;
    const size_t plane = (sn + 3) & ~size_t(3);
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_compact_gather, dim3(sc_blocks(take, int64_t(1) << 31)), dim3(kScBlock), 0, ctx->stream, ctx->s_cell.p, take,
                         ctx->xyz.p, ctx->xyz.p + plane, ctx->xyz.p + 2 * plane, packed, out_label ? ctx->labels.p : nullptr,
                         out_xyz ? d_xyz : nullptr, out_rgb ? d_rgb : nullptr, out_label ? d_label : nullptr);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    if (out_xyz) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_xyz, d_xyz, 12 * st, hipMemcpyDeviceToHost, ctx->stream));
    if (out_rgb) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rgb, d_rgb, 3 * st, hipMemcpyDeviceToHost, ctx->stream));
    if (out_label) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_label, d_label, st, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (out_index) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_index, ctx->s_cell.p, 4 * st, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

}  // extern "C"
