// pcp_ortho_texture.hip -- orthophotos ("Orthophotos", OT1-OT9): the finished orthographic map walked at a finer
// pitch, a surface point behind every fine pixel (pcp_ortho_texture.hpp), coloured straight from the keyframe images by the
// code the colour pass runs on map points: project_point, keep_rule against the context's depth maps, final_score,
// Top5.  One lane per fine pixel, one 16 x 16 tile per workgroup; the keyframe loop is wave-uniform, and before it the
// workgroup lists the keyframes that can see its tile at all (tile_classify on the tile's bounding sphere).
// A cylinder's unrolled map ("Orthophotos of unrolled maps", CT1-CT8) differs in the surface point alone (pcp_ortho_cyl.hpp).
// Opt-in: nothing here runs unless pcp_ortho_texture or pcp_ortho_texture_cyl is called.  Build with -ffp-contract=off (see
// pcp_device.hpp).
#include <algorithm>
#include <cmath>
#include <new>

#include "pcp_device.hpp"
#include "pcp_ortho_cyl.hpp"
#include "pcp_ortho_texture.hpp"
#include "pcp_tile_classify.hpp"

namespace pcp {

constexpr int kOtTile = 16;
constexpr int kOtBlock = kOtTile * kOtTile;
constexpr int kOtWaves = kOtBlock / 64;
constexpr int kOtMaxWords = (ot::kMaxFrames + 31) / 32;
enum { OT_SURFACE = 0, OT_TEXTURED, OT_UNSEEN, OT_SKIPPED, OT_SCALARS };

// the finished map as the kernel reads it: a plane's frame, or a cylinder's (kCyl, CT4)
struct OtPlane {
  float o[3], u[3], v[3], n[3];
  float gsd;
};
template <bool kCyl>
struct OtMap {
  std::conditional_t<kCyl, cy::Frame, OtPlane> f;
  int32_t W, H;
  const int32_t *source;
  const unsigned long long *keys;
};
// the layers a call asked for (nullptr: not asked), device memory
struct OtOut {
  uint8_t *rgb, *mask, *status, *count;
  int16_t *view;
};

__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// OT6: a listed view's word with its channels under the view's gain (the mask byte stays)
__device__ __forceinline__ uint32_t ot_gained(uint32_t c, int32_t f, const float *__restrict__ gains) {
  if (f < 0) return c;
  const float g = gains[f];
  return (c & 0xff000000u) | (gained_channel((c >> 16) & 0xffu, g) << 16) | (gained_channel((c >> 8) & 0xffu, g) << 8) |
         gained_channel(c & 0xffu, g);
}

// OT3-OT7.  Lane (lx, ly) of workgroup (bx, by) is fine pixel (16 bx + lx, 16 by + ly) of the call's raster.
// kCyl: the surface point is CT2's, and a pixel whose rho is not above 0 has no surface; all else is the same.
template <bool kCyl>
__global__ __launch_bounds__(kOtBlock) void k_ortho_texture(ot::Raster r, OtMap<kCyl> m, DevCamera cam, const DevFrame *__restrict__ frames,
                                                            int32_t n_frames, const uint32_t *__restrict__ depth, int64_t cells,
                                                            const uint32_t *__restrict__ images, int64_t image_px,
                                                            const float *__restrict__ gains, int32_t views, OtOut out,
                                                            unsigned long long *__restrict__ scalars) {
  __shared__ float s_box[kOtWaves][6];
  __shared__ float s_far[kOtWaves];
  __shared__ uint32_t s_bits[kOtMaxWords];
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int32_t fw = r.w * r.k, fh = r.h * r.k;
  const int32_t X = static_cast<int32_t>(blockIdx.x) * kOtTile + (tid & (kOtTile - 1));
  const int32_t Y = static_cast<int32_t>(blockIdx.y) * kOtTile + (tid >> 4);
  const bool inside = X < fw && Y < fh;
  // OT3
  float p[3] = {0.0f, 0.0f, 0.0f};
  bool surface = false;
  if (inside) {
    const int32_t Xg = r.x0 * r.k + X, Yg = r.y0 * r.k + Y;
    float d;
    surface = ot::surface_depth(r, m.W, m.H, m.source, [&](int32_t s) { return om::key_depth(m.keys[s]); }, Xg, Yg, &d);
    if constexpr (kCyl) {
      if (surface) surface = cy::surface_point(m.f, r.k, Xg, Yg, d, p);
    } else {
      if (surface) ot::surface_point(m.f.o, m.f.u, m.f.v, m.f.n, m.f.gsd, r.k, Xg, Yg, d, p);
    }
  }
  // OT7: the tile's bounding sphere -- the centre of its surface points' box, the largest distance from it
  {
    const float inf = __builtin_inff();
    const float lo0 = wave_min_f32(surface ? p[0] : inf), lo1 = wave_min_f32(surface ? p[1] : inf), lo2 = wave_min_f32(surface ? p[2] : inf);
    const float hi0 = wave_max_f32(surface ? p[0] : -inf), hi1 = wave_max_f32(surface ? p[1] : -inf), hi2 = wave_max_f32(surface ? p[2] : -inf);
    if (lane == 0) {
      s_box[wave][0] = lo0; s_box[wave][1] = lo1; s_box[wave][2] = lo2;
      s_box[wave][3] = hi0; s_box[wave][4] = hi1; s_box[wave][5] = hi2;
    }
  }
  __syncthreads();
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = fminf(fminf(s_box[0][a], s_box[1][a]), fminf(s_box[2][a], s_box[3][a]));
    hi[a] = fmaxf(fmaxf(s_box[0][a + 3], s_box[1][a + 3]), fmaxf(s_box[2][a + 3], s_box[3][a + 3]));
  }
  const bool any_surface = lo[0] <= hi[0];  // (the same in every lane of the workgroup)
  Top5 t;
  t.init();
  if (any_surface) {
    float4 sph;
    sph.x = 0.5f * lo[0] + 0.5f * hi[0];
    sph.y = 0.5f * lo[1] + 0.5f * hi[1];
    sph.z = 0.5f * lo[2] + 0.5f * hi[2];
    {
      const float dx = p[0] - sph.x, dy = p[1] - sph.y, dz = p[2] - sph.z;
      const float far = wave_max_f32(surface ? sqrtf((dx * dx + dy * dy) + dz * dz) : 0.0f);
      if (lane == 0) s_far[wave] = far;
    }
    __syncthreads();
    // (the fp32 distance is within a few ulp of the real one: a part in 10^5 and the smallest normal cover it; a point that
    // is not finite makes the centre or the radius non-finite, and tile_classify then keeps every keyframe)
    sph.w = fmaxf(fmaxf(s_far[0], s_far[1]), fmaxf(s_far[2], s_far[3])) * 1.00001f + 1.17549435e-38f;
    // the keyframes that may see the tile, one bit each: lane j of a pass tests keyframe base + j, a half wavefront's ballot is a word
    const int32_t words = (n_frames + 31) >> 5;
    for (int32_t base = 0; base < n_frames; base += kOtBlock) {
      const int32_t f = base + tid;
      const bool may = f < n_frames && tile_classify(cam, frames[f], sph) != 1;
      const unsigned long long b = __ballot(may);
      const int32_t w = (base >> 5) + 2 * wave + (lane >> 5);
      if ((lane & 31) == 0 && w < words) s_bits[w] = static_cast<uint32_t>(lane ? b >> 32 : b);
    }
    __syncthreads();
    // OT4: the listed keyframes ascending; f is the same in every lane, so DevFrame comes through the scalar cache
    uint32_t walked = 0u;
    for (int32_t w = 0; w < words; ++w) {
      uint32_t todo = __builtin_amdgcn_readfirstlane(s_bits[w]);
      walked += __popc(todo);
      while (todo) {
        const int32_t f = (w << 5) + __builtin_ctz(todo);
        todo &= todo - 1u;
        const DevFrame &fr = frames[f];
        const Projected q = project_point<true, false>(cam, fr.w2c, p[0], p[1], p[2]);
        // (cells and image_px are below 2^31, f is not negative: see k_colour_pass)
        if (surface && q.pixel >= 0 && keep_rule(cam, q, depth + static_cast<uint64_t>(static_cast<uint32_t>(f)) * static_cast<uint32_t>(cells))) {
          const uint32_t texel = images[static_cast<uint64_t>(static_cast<uint32_t>(f)) * static_cast<uint32_t>(image_px) + static_cast<uint32_t>(q.pixel)];
          t.insert(final_score(q.xc, q.yc, q.zc, fr.px, fr.py, fr.pz), texel, f);
        }
      }
    }
    if (tid == 0 && walked < static_cast<uint32_t>(n_frames))
      atomicAdd(scalars + OT_SKIPPED, static_cast<unsigned long long>(static_cast<uint32_t>(n_frames) - walked));
  }
  // OT5
  const bool textured = t.count >= 1;
  const unsigned long long ns = __popcll(__ballot(surface)), nt = __popcll(__ballot(textured));
  if (lane == 0 && ns) {
    atomicAdd(scalars + OT_SURFACE, ns);
    if (nt) atomicAdd(scalars + OT_TEXTURED, nt);
    if (ns > nt) atomicAdd(scalars + OT_UNSEEN, ns - nt);
  }
  if (!inside) return;
  uint32_t word = 0u;
  if (textured) {
    Top5 q = t;
    if (gains) {  // OT6
      q.c0 = ot_gained(q.c0, q.f0, gains);
      q.c1 = ot_gained(q.c1, q.f1, gains);
      q.c2 = ot_gained(q.c2, q.f2, gains);
      q.c3 = ot_gained(q.c3, q.f3, gains);
      q.c4 = ot_gained(q.c4, q.f4, gains);
    }
    // the first min(count, views) entries: finalise sums the entries that name a keyframe
    if (views < 5) q.f4 = -1;
    if (views < 4) q.f3 = -1;
    if (views < 3) q.f2 = -1;
    if (views < 2) q.f1 = -1;
    word = q.finalise();
  }
  const int64_t at = static_cast<int64_t>(Y) * fw + X;
  if (out.rgb) {
    out.rgb[3 * at] = static_cast<uint8_t>(word);
    out.rgb[3 * at + 1] = static_cast<uint8_t>(word >> 8);
    out.rgb[3 * at + 2] = static_cast<uint8_t>(word >> 16);
  }
  if (out.mask) out.mask[at] = textured ? static_cast<uint8_t>(t.c0 >> 24) : 0;
  if (out.status) out.status[at] = surface ? (textured ? 1 : 2) : 0;
  if (out.view) out.view[at] = textured ? static_cast<int16_t>(t.f0) : static_cast<int16_t>(-1);
  if (out.count) out.count[at] = static_cast<uint8_t>(t.count < 255 ? t.count : 255);
}

hipError_t preload_ortho_texture() {
  hipFuncAttributes a;
  const hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_ortho_texture<false>));
  return e != hipSuccess ? e : hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_ortho_texture<true>));
}

// OT2 for either form: the resolved raster, or the refusal in msg
static int ot_check_raster(const char *who, int32_t W, int32_t H, const pcp_ortho_texture_params &p, ot::Raster *r, char *msg, size_t cap) {
  const char *why = "";
  int32_t fit = 0;
  const int bad = ot::raster_check(W, H, p.scale, p.x0, p.y0, p.w, p.h, p.views, p.interpolate, p.max_step, r, &why, &fit);
  if (bad == 1) {
    std::snprintf(msg, cap, "%s: %s (scale %d, rectangle %d %d %d x %d of %d x %d, views %d, max_step %g)", who, why, p.scale, p.x0, p.y0,
                  p.w, p.h, W, H, p.views, static_cast<double>(p.max_step));
    return PCP_ERR_INVALID;
  }
  if (bad == 2) {
    std::snprintf(msg, cap, "%s: %s at scale %d; the largest scale that fits the rectangle is %d", who, why, p.scale, fit);
    return PCP_ERR_RANGE;
  }
  return PCP_OK;
}

// pcp_ortho_texture (kCyl false) and pcp_ortho_texture_cyl (true): OT1's checks in OT1's order, OT2, the launch, the copies
template <bool kCyl>
static int ot_texture(pcp_context *ctx, const char *who, const pcp_ortho_texture_params *params, uint8_t *out_rgb, uint8_t *out_mask,
                      uint8_t *out_status, int16_t *out_view, uint8_t *out_count, int64_t out_counts[4]) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
  if (!params) return set_error(ctx, PCP_ERR_INVALID, "%s: NULL params", who);
  // OT1
  const OrthoMap &m = ctx->ortho;
  if (!m.live) return set_error(ctx, PCP_ERR_STATE, "%s: no orthographic map (call pcp_ortho_begin)", who);
  if (!kCyl && m.cyl)  // CY4, CT5
    return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_texture: the live map is a cylinder's unrolled map (pcp_ortho_begin_cyl); orthophotos "
                     "of unrolled maps are not built by this call (pcp_ortho_texture_cyl builds them)");
  if (kCyl && !m.cyl)
    return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_texture_cyl: the live map is a plane's (pcp_ortho_begin); pcp_ortho_texture builds "
                     "its orthophoto");
  if (!m.finished) return set_error(ctx, PCP_ERR_STATE, "%s: pcp_ortho_finish has not run", who);
  if (!ctx->have_camera) return set_error(ctx, PCP_ERR_STATE, "%s: pcp_set_camera has not been called", who);
  const int32_t F = ctx->n_frames;
  if (F <= 0) return set_error(ctx, PCP_ERR_STATE, "%s: pcp_set_frames has not been called", who);
  if (F > ot::kMaxFrames)  // (OT2, with the keyframes: before their images are asked for)
    return set_error(ctx, PCP_ERR_RANGE, "%s: %d keyframes, the view layer (int16) names at most %d", who, F, ot::kMaxFrames);
  if (ctx->dcam.cull_mode != PCP_CULL_ZBUFFER || !ctx->dcam.enable_zbuf)
    return set_error(ctx, PCP_ERR_STATE, "%s: needs PCP_CULL_ZBUFFER with the depth buffer on (a surface point is kept or dropped by "
                     "the depth maps; PCP_CULL_HPR* has none)", who);
  for (size_t f = 0; f < static_cast<size_t>(F); ++f)
    if (!ctx->images.p || f >= ctx->image_set.size() || !ctx->image_set[f])
      return set_error(ctx, PCP_ERR_STATE, "%s: no image uploaded for keyframe %d", who, static_cast<int>(f));
  for (size_t f = 0; f < static_cast<size_t>(F); ++f)
    if (!ctx->depth.p || f >= ctx->depth_valid.size() || !ctx->depth_valid[f])
      return set_error(ctx, PCP_ERR_STATE, "%s: pcp_depth_pass has not covered keyframe %d since the latest upload", who,
                       static_cast<int>(f));
  // OT2
  ot::Raster r{};
  char msg[320];
  const int rc = ot_check_raster(who, m.frame.width, m.frame.height, *params, &r, msg, sizeof msg);
  if (rc != PCP_OK) return set_error(ctx, rc, "%s", msg);
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int wrc = wait_images(ctx, 0, F);
  if (wrc != PCP_OK) return wrc;
  const int32_t fw = r.w * r.k, fh = r.h * r.k;
  const size_t px = static_cast<size_t>(fw) * static_cast<size_t>(fh);
  // OT8: 8 B per fine pixel when every layer is asked for, gone on return
  DevBuf<uint8_t> d_rgb, d_mask, d_status, d_count;
  DevBuf<int16_t> d_view;
  DevBuf<unsigned long long> d_scalars;
  if (out_rgb) PCP_HIP_TRY(ctx, d_rgb.ensure(3 * px));
  if (out_mask) PCP_HIP_TRY(ctx, d_mask.ensure(px));
  if (out_status) PCP_HIP_TRY(ctx, d_status.ensure(px));
  if (out_count) PCP_HIP_TRY(ctx, d_count.ensure(px));
  if (out_view) PCP_HIP_TRY(ctx, d_view.ensure(px));
  PCP_HIP_TRY(ctx, d_scalars.ensure(OT_SCALARS));
  PCP_HIP_TRY(ctx, hipMemsetAsync(d_scalars.p, 0, OT_SCALARS * 8, ctx->stream));
  OtMap<kCyl> dm;
  if constexpr (kCyl) {
    dm.f = cy::make_frame(m.cyl_frame);
  } else {
    for (int a = 0; a < 3; ++a) {
      dm.f.o[a] = m.frame.o[a];
      dm.f.u[a] = m.frame.u[a];
      dm.f.v[a] = m.frame.v[a];
      dm.f.n[a] = m.frame.n[a];
    }
    dm.f.gsd = m.frame.gsd;
  }
  dm.W = m.frame.width;
  dm.H = m.frame.height;
  dm.source = m.source.p;
  dm.keys = m.keys.p;
  const OtOut out{d_rgb.p, d_mask.p, d_status.p, d_count.p, d_view.p};
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    const dim3 grid(static_cast<uint32_t>(div_up(fw, kOtTile)), static_cast<uint32_t>(div_up(fh, kOtTile)));
    hipLaunchKernelGGL(k_ortho_texture<kCyl>, grid, dim3(kOtBlock), 0, ctx->stream, r, dm, ctx->dcam, ctx->frames.p, F, ctx->depth.p,
                       static_cast<int64_t>(ctx->dcam.mw) * ctx->dcam.mh, ctx->images.p,
                       static_cast<int64_t>(ctx->dcam.img_w) * ctx->dcam.img_h, ctx->gains_set ? ctx->gains_dev.p : static_cast<const float *>(nullptr),
                       params->views, out, d_scalars.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  unsigned long long h[OT_SCALARS];
  if (out_rgb) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rgb, d_rgb.p, 3 * px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_mask) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_mask, d_mask.p, px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_status) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_status, d_status.p, px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_count) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_count, d_count.p, px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_view) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_view, d_view.p, 2 * px, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(h, d_scalars.p, OT_SCALARS * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the layers' device copies are freed on return)
  if (out_counts)
    for (int k = 0; k < OT_SCALARS; ++k) out_counts[k] = static_cast<int64_t>(h[k]);
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_ortho_texture(pcp_context *ctx, const pcp_ortho_texture_params *params, uint8_t *out_rgb, uint8_t *out_mask, uint8_t *out_status,
                      int16_t *out_view, uint8_t *out_count, int64_t out_counts[4]) {
  return ot_texture<false>(ctx, "pcp_ortho_texture", params, out_rgb, out_mask, out_status, out_view, out_count, out_counts);
}

int pcp_ortho_texture_cyl(pcp_context *ctx, const pcp_ortho_texture_params *params, uint8_t *out_rgb, uint8_t *out_mask, uint8_t *out_status,
                          int16_t *out_view, uint8_t *out_count, int64_t out_counts[4]) {
  return ot_texture<true>(ctx, "pcp_ortho_texture_cyl", params, out_rgb, out_mask, out_status, out_view, out_count, out_counts);
}

int pcp_ortho_texture_points_host(const pcp_ortho_frame *frame, const pcp_ortho_texture_params *params, const int32_t *source,
                                  const float *depth, float *out_xyz, uint8_t *out_ok) {
  if (!frame || !params || !source || !depth) {
    set_global_error("pcp_ortho_texture_points_host: NULL frame, params, source or depth");
    return PCP_ERR_INVALID;
  }
  const char *why = "";
  double fit = 0.0;
  const int bad = om::frame_check(frame->o, frame->u, frame->v, frame->n, frame->gsd, frame->width, frame->height, frame->d_min,
                                  frame->d_max, &why, &fit);
  if (bad) {
    set_global_error("pcp_ortho_texture_points_host: %s", why);
    return bad == 1 ? PCP_ERR_INVALID : PCP_ERR_RANGE;
  }
  ot::Raster r{};
  char msg[320];
  const int rc = ot_check_raster("pcp_ortho_texture_points_host", frame->width, frame->height, *params, &r, msg, sizeof msg);
  if (rc != PCP_OK) {
    set_global_error("%s", msg);
    return rc;
  }
  const int32_t W = frame->width, H = frame->height, fw = r.w * r.k, fh = r.h * r.k;
  const int64_t map_px = static_cast<int64_t>(W) * H;
  for (int64_t q = 0; q < map_px; ++q)
    if (source[q] >= map_px) {
      set_global_error("pcp_ortho_texture_points_host: source[%lld] = %d names no pixel of the %d x %d map", static_cast<long long>(q),
                       source[q], W, H);
      return PCP_ERR_INVALID;
    }
  for (int32_t Y = 0; Y < fh; ++Y)
    for (int32_t X = 0; X < fw; ++X) {
      const int32_t Xg = r.x0 * r.k + X, Yg = r.y0 * r.k + Y;
      float d = 0.0f, p[3] = {0.0f, 0.0f, 0.0f};
      const bool ok = ot::surface_depth(r, W, H, source, [&](int32_t s) { return depth[s]; }, Xg, Yg, &d);
      if (ok) ot::surface_point(frame->o, frame->u, frame->v, frame->n, frame->gsd, r.k, Xg, Yg, d, p);
      const int64_t at = static_cast<int64_t>(Y) * fw + X;
      if (out_xyz)
        for (int a = 0; a < 3; ++a) out_xyz[3 * at + a] = p[a];
      if (out_ok) out_ok[at] = ok ? 1 : 0;
    }
  return PCP_OK;
}

int pcp_ortho_texture_points_cyl_host(const pcp_cyl_frame *frame, const pcp_ortho_texture_params *params, const int32_t *source,
                                      const float *depth, float *out_xyz, uint8_t *out_ok) {
  const char *who = "pcp_ortho_texture_points_cyl_host";
  if (!frame || !params || !source || !depth) {
    set_global_error("%s: NULL frame, params, source or depth", who);
    return PCP_ERR_INVALID;
  }
  const char *why = "";
  double fit = 0.0;
  const int bad = cy::frame_check(frame->c, frame->a, frame->e, frame->b, frame->radius, frame->gsd, frame->width, frame->height,
                                  frame->d_min, frame->d_max, frame->side, &why, &fit);
  if (bad) {
    set_global_error("%s: %s", who, why);
    return bad == 1 ? PCP_ERR_INVALID : PCP_ERR_RANGE;
  }
  ot::Raster r{};
  char msg[320];
  const int rc = ot_check_raster(who, frame->width, frame->height, *params, &r, msg, sizeof msg);
  if (rc != PCP_OK) {
    set_global_error("%s", msg);
    return rc;
  }
  const int32_t W = frame->width, H = frame->height, fw = r.w * r.k, fh = r.h * r.k;
  const int64_t map_px = static_cast<int64_t>(W) * H;
  for (int64_t q = 0; q < map_px; ++q)
    if (source[q] >= map_px) {
      set_global_error("%s: source[%lld] = %d names no pixel of the %d x %d map", who, static_cast<long long>(q), source[q], W, H);
      return PCP_ERR_INVALID;
    }
  const cy::Frame f = cy::make_frame(*frame);
  for (int32_t Y = 0; Y < fh; ++Y)
    for (int32_t X = 0; X < fw; ++X) {
      const int32_t Xg = r.x0 * r.k + X, Yg = r.y0 * r.k + Y;
      float d = 0.0f, p[3] = {0.0f, 0.0f, 0.0f};
      bool ok = ot::surface_depth(r, W, H, source, [&](int32_t s) { return depth[s]; }, Xg, Yg, &d);
      if (ok) ok = cy::surface_point(f, r.k, Xg, Yg, d, p);  // (false: rho <= 0, p stays 0)
      const int64_t at = static_cast<int64_t>(Y) * fw + X;
      if (out_xyz)
        for (int a = 0; a < 3; ++a) out_xyz[3 * at + a] = p[a];
      if (out_ok) out_ok[at] = ok ? 1 : 0;
    }
  return PCP_OK;
}

int pcp_cyl_sincos_host(int64_t n, const double *theta, double *out_sin, double *out_cos) {
  if (n < 0 || (n > 0 && (!theta || !out_sin || !out_cos))) {
    set_global_error("pcp_cyl_sincos_host: negative n or a NULL array");
    return PCP_ERR_INVALID;
  }
  for (int64_t i = 0; i < n; ++i)
    if (!(theta[i] >= 0.0 && theta[i] < 64.0)) {  // (a NaN fails both)
      set_global_error("pcp_cyl_sincos_host: theta[%lld] = %g is outside [0, 64) or not finite", static_cast<long long>(i), theta[i]);
      return PCP_ERR_INVALID;
    }
  for (int64_t i = 0; i < n; ++i) cy::sincos(theta[i], out_sin + i, out_cos + i);
  return PCP_OK;
}

}  // extern "C"
