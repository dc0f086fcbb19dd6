// pcp_image_balance.hip -- keyframe colour balance at upload: CLAHE on V and a gamma table ("Image balance",
// IB1-IB9), replacing the reference's scripts/image_color_balance_autonomous.py / image_color_balance.py run over the keyframe
// folder.  The arithmetic is pcp_image_balance.hpp's; this file holds the three kernels, their launch on an upload lane
// (upload_texels in pcp_colour.hip calls balance_texels behind the source's pack kernel, so decoded BGR, pinned blocks and
// device JPEG are one path), the host twin and the stand-alone device form.
//
//   k_balance_hist   per-tile histograms of V over the extended tile, several workgroups per tile: a sub-histogram per
//                    wavefront in LDS, one add for a wavefront whose lanes all hold the same V (flat regions), the non-zero
//                    bins merged into the tile's global histogram by integer adds (order-independent)
//   k_balance_lut    one workgroup per tile, one lane per bin: clipped sum and inclusive prefix sum by LDS scans, the
//                    redistribution in closed form, the table byte; leaves the histogram zeroed for the lane's next image
//   k_balance_apply  per pixel: HSV forward, four table reads from LDS (the two tile rows and the few tile columns the
//                    workgroup's row segment touches, at most 8 KB), interpolation, HSV backward, gamma table from LDS,
//                    pcp_set_image_adjust's round trip when enabled; the mask byte is kept; 16-B loads and stores when
//                    the width is a multiple of 4
#include <algorithm>
#include <cmath>
#include <vector>

#include "pcp_image_balance.hpp"
#include "pcp_internal.hpp"

namespace pcp {

constexpr int kIbBlock = 256;
constexpr int kIbWaves = kIbBlock / 64;
constexpr int32_t kHistChunk = kIbBlock * 8;  // extended pixels of one tile per workgroup (8192: 15.5 instead of 6.2 us at 1080p)
constexpr size_t kHistWords = static_cast<size_t>(ib::kMaxTiles) * ib::kMaxTiles * ib::kBins;
constexpr size_t kLutBytes = kHistWords;  // the gamma table follows at this offset
constexpr int32_t kIbMaxSide = 16384;
constexpr int64_t kIbMaxPixels = int64_t(1) << 26;

__device__ __forceinline__ uint32_t texel_v(uint32_t t) {  // V of RGB2HSV_b: the largest of B, G, R
  const uint32_t b = t & 0xffu, g = (t >> 8) & 0xffu, r = (t >> 16) & 0xffu;
  const uint32_t m = b > g ? b : g;
  return m > r ? m : r;
}

__global__ __launch_bounds__(kIbBlock) void k_balance_hist(const uint32_t *__restrict__ texels, ib::Grid g,
                                                            uint32_t *__restrict__ hist) {
  __shared__ uint32_t sub[kIbWaves][ib::kBins];
  const int32_t tile = static_cast<int32_t>(blockIdx.y);
  const int32_t ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
  for (int i = threadIdx.x; i < kIbWaves * ib::kBins; i += kIbBlock) (&sub[0][0])[i] = 0u;
  __syncthreads();
  const int32_t p0 = static_cast<int32_t>(blockIdx.x) * kHistChunk;
  const int32_t p1 = min(p0 + kHistChunk, g.total);
  uint32_t *mine = sub[threadIdx.x >> 6];
  for (int32_t p = p0 + static_cast<int32_t>(threadIdx.x); p < p1; p += kIbBlock) {
    const int32_t row = p / g.tw, col = p - row * g.tw;
    const int32_t x = ib::reflect101(tx * g.tw + col, g.w), y = ib::reflect101(ty * g.th + row, g.h);
    const uint32_t v = texel_v(texels[static_cast<int64_t>(y) * g.w + x]);
    // a flat region sends the whole wavefront to one bin: one add of the lane count instead of 64 serialised ones
    const uint32_t first = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
    const unsigned long long active = __ballot(1), same = __ballot(v == first);
    if (same == active) {
      if (static_cast<unsigned>(__lane_id()) == static_cast<unsigned>(__ffsll(static_cast<long long>(active)) - 1))
        atomicAdd(&mine[first], static_cast<uint32_t>(__popcll(active)));
    } else {
      atomicAdd(&mine[v], 1u);
    }
  }
  __syncthreads();
  uint32_t sum = 0;
#pragma unroll
  for (int w = 0; w < kIbWaves; ++w) sum += sub[w][threadIdx.x];
  if (sum) atomicAdd(&hist[static_cast<int64_t>(tile) * ib::kBins + threadIdx.x], sum);
}

// inclusive prefix sum over the workgroup's 256 values
__device__ __forceinline__ int32_t scan256(int32_t v, int32_t *s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < kIbBlock; off <<= 1) {
    const int32_t t = static_cast<int>(threadIdx.x) >= off ? s[threadIdx.x - off] : 0;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  return s[threadIdx.x];
}

__global__ __launch_bounds__(kIbBlock) void k_balance_lut(uint32_t *__restrict__ hist, ib::Grid g, int32_t clip,
                                                           uint8_t *__restrict__ lut) {
  __shared__ int32_t s[kIbBlock];
  const int64_t at = static_cast<int64_t>(blockIdx.x) * ib::kBins + threadIdx.x;
  const int32_t count = static_cast<int32_t>(hist[at]);
  hist[at] = 0u;
  (void)scan256(ib::excess(count, clip), s);
  const int32_t clipped = s[kIbBlock - 1];
  __syncthreads();
  const int32_t cum = scan256(ib::redistributed(count, static_cast<int32_t>(threadIdx.x), clip, clipped), s);
  lut[at] = static_cast<uint8_t>(ib::lut_entry(cum, g.lut_scale));
}

struct BalanceApplyArgs {
  ib::Grid g;
  int32_t w, h;
  int32_t clahe, gamma, adjust;
  float sat_scale, val_scale;
};

template <int VEC>
__global__ __launch_bounds__(kIbBlock) void k_balance_apply(uint32_t *__restrict__ texels, BalanceApplyArgs a,
                                                             const uint8_t *__restrict__ lut,
                                                             const uint8_t *__restrict__ gamma_table,
                                                             const int32_t *__restrict__ hsv_tables) {
  __shared__ uint32_t s_lut32[2 * ib::kMaxTiles * ib::kBins / 4];
  __shared__ uint32_t s_gamma32[ib::kBins / 4];
  const uint8_t *s_lut = reinterpret_cast<const uint8_t *>(s_lut32);
  const uint8_t *s_gamma = reinterpret_cast<const uint8_t *>(s_gamma32);
  const int32_t y = static_cast<int32_t>(blockIdx.y);
  const int32_t x0 = static_cast<int32_t>(blockIdx.x) * (kIbBlock * VEC);
  ib::Weights wy{};
  int32_t c0 = 0;
  if (a.clahe) {
    // the tile columns this row segment can touch: floor(x / tw - 0.5) >= x / tw - 1 and its successor <= x / tw + 1
    const int32_t x1 = min(x0 + kIbBlock * VEC, a.w) - 1;
    c0 = max(x0 / a.g.tw - 1, 0);
    const int32_t c1 = min(x1 / a.g.tw + 1, a.g.tiles_x - 1);
    const int32_t words = (c1 - c0 + 1) * (ib::kBins / 4);
    wy = ib::weights(y, a.g.inv_th, a.g.tiles_y);
    const uint32_t *r1 = reinterpret_cast<const uint32_t *>(lut + (static_cast<int64_t>(wy.t1) * a.g.tiles_x + c0) * ib::kBins);
    const uint32_t *r2 = reinterpret_cast<const uint32_t *>(lut + (static_cast<int64_t>(wy.t2) * a.g.tiles_x + c0) * ib::kBins);
    for (int32_t i = threadIdx.x; i < words; i += kIbBlock) {
      s_lut32[i] = r1[i];
      s_lut32[ib::kMaxTiles * ib::kBins / 4 + i] = r2[i];
    }
  }
  if (a.gamma && threadIdx.x < ib::kBins / 4) s_gamma32[threadIdx.x] = reinterpret_cast<const uint32_t *>(gamma_table)[threadIdx.x];
  __syncthreads();
  const int32_t x = x0 + static_cast<int32_t>(threadIdx.x) * VEC;
  if (x >= a.w) return;  // (VEC == 4 only with w % 4 == 0: a lane's four pixels are all inside or all outside)
  uint32_t *at = texels + static_cast<int64_t>(y) * a.w + x;
  uint32_t px[VEC];
  if constexpr (VEC == 4) {
    const uint4 q = *reinterpret_cast<const uint4 *>(at);
    px[0] = q.x;
    px[1] = q.y;
    px[2] = q.z;
    px[3] = q.w;
  } else {
    px[0] = *at;
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    uint32_t b = px[k] & 0xffu, gg = (px[k] >> 8) & 0xffu, r = (px[k] >> 16) & 0xffu;
    if (a.clahe) {
      uint32_t H, S, V;
      hsv_forward(hsv_tables, hsv_tables + 256, b, gg, r, H, S, V);
      ib::Weights wx = ib::weights(x + k, a.g.inv_tw, a.g.tiles_x);
      const uint8_t *l1 = s_lut + (wx.t1 - c0) * ib::kBins + V, *l2 = s_lut + (wx.t2 - c0) * ib::kBins + V;
      const uint32_t v2 = ib::interpolate(l1[0], l2[0], l1[ib::kMaxTiles * ib::kBins], l2[ib::kMaxTiles * ib::kBins], wx, wy);
      hsv_backward(H, S, v2, b, gg, r);
    }
    if (a.gamma) {
      b = s_gamma[b];
      gg = s_gamma[gg];
      r = s_gamma[r];
    }
    if (a.adjust) hsv_round_trip(hsv_tables, hsv_tables + 256, a.sat_scale, a.val_scale, b, gg, r);
    px[k] = (px[k] & 0xff000000u) | b | (gg << 8) | (r << 16);
  }
  if constexpr (VEC == 4)
    *reinterpret_cast<uint4 *>(at) = make_uint4(px[0], px[1], px[2], px[3]);
  else
    *at = px[0];
}

// pcp_image_balance: texels -> tightly packed BGR8
__global__ __launch_bounds__(kIbBlock) void k_balance_unpack(const uint32_t *__restrict__ texels, int64_t n, uint8_t *__restrict__ bgr) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kIbBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t t = texels[i];
  bgr[3 * i] = static_cast<uint8_t>(t);
  bgr[3 * i + 1] = static_cast<uint8_t>(t >> 8);
  bgr[3 * i + 2] = static_cast<uint8_t>(t >> 16);
}

// nullptr: the parameters are fine
static const char *balance_params_fault(const pcp_balance_params *p) {
  if ((p->stages & ~(PCP_BALANCE_CLAHE | PCP_BALANCE_GAMMA)) != 0) return "unknown stage bits";
  if (p->tiles_x < 1 || p->tiles_x > ib::kMaxTiles || p->tiles_y < 1 || p->tiles_y > ib::kMaxTiles) return "tiles outside 1..16";
  if (!std::isfinite(p->clip_limit)) return "clip limit not finite";
  if (!std::isfinite(p->gamma) || !(p->gamma > 0.0f)) return "gamma must be finite and > 0";
  return nullptr;
}

struct BalanceTimed {  // a LaunchTimer only on the context's own stream
  LaunchTimer t;
  BalanceTimed(pcp_context *ctx, bool on) : t(on ? ctx : nullptr, PCP_K_MISC) {}
};

hipError_t preload_image_balance() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_balance_hist));
}

int balance_check(pcp_context *ctx, const char *who, const pcp_balance_params &p, int32_t w, int32_t h) {
  if (w > kIbMaxSide || h > kIbMaxSide)
    return set_error(ctx, PCP_ERR_RANGE, "%s: image balance: a side of %d x %d above %d", who, w, h, kIbMaxSide);
  if (!(p.stages & PCP_BALANCE_CLAHE)) return PCP_OK;
  ib::Grid g;
  if (ib::make_grid(w, h, p.tiles_x, p.tiles_y, &g) != 0)
    return set_error(ctx, PCP_ERR_RANGE, "%s: image balance: a %d x %d image cannot be extended to %d x %d tiles by reflection (IB3)", who,
                     w, h, p.tiles_x, p.tiles_y);
  return PCP_OK;
}

int balance_scratch(pcp_context *ctx, int lane, hipStream_t s) {
  if (!ctx->balance_hist[lane].p) {
    PCP_HIP_TRY(ctx, ctx->balance_hist[lane].ensure(kHistWords));
    PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->balance_hist[lane].p, 0, kHistWords * sizeof(uint32_t), s));  // from here on k_balance_lut's job
  }
  PCP_HIP_TRY(ctx, ctx->balance_lut[lane].ensure(kLutBytes + ib::kBins));
  return PCP_OK;
}

int balance_texels(pcp_context *ctx, int lane, hipStream_t s, const BalanceRun &run, int32_t w, int32_t h, uint32_t *texels) {
  const pcp_balance_params &p = run.params;
  uint32_t *hist = ctx->balance_hist[lane].p;
  uint8_t *lut = ctx->balance_lut[lane].p, *gamma = lut + kLutBytes;
  BalanceApplyArgs a{};
  a.w = w;
  a.h = h;
  a.clahe = (p.stages & PCP_BALANCE_CLAHE) ? 1 : 0;
  a.gamma = (p.stages & PCP_BALANCE_GAMMA) ? 1 : 0;
  a.adjust = run.adjust ? 1 : 0;
  a.sat_scale = run.sat_scale;
  a.val_scale = run.val_scale;
  if (a.gamma && run.gamma_stale) PCP_HIP_TRY(ctx, hipMemcpyAsync(gamma, run.gamma_host, ib::kBins, hipMemcpyHostToDevice, s));
  if (a.clahe) {
    if (ib::make_grid(w, h, p.tiles_x, p.tiles_y, &a.g) != 0) return set_error(ctx, PCP_ERR_RANGE, "image balance: tile grid (IB3)");
    const int32_t tiles = p.tiles_x * p.tiles_y;
    {
      BalanceTimed t(ctx, run.timed);
      hipLaunchKernelGGL(k_balance_hist, dim3(static_cast<uint32_t>(div_up(a.g.total, kHistChunk)), static_cast<uint32_t>(tiles)),
                         dim3(kIbBlock), 0, s, texels, a.g, hist);
    }
    if (run.out_hist)
      PCP_HIP_TRY(ctx, hipMemcpyAsync(run.out_hist, hist, static_cast<size_t>(tiles) * ib::kBins * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    {
      BalanceTimed t(ctx, run.timed);
      hipLaunchKernelGGL(k_balance_lut, dim3(static_cast<uint32_t>(tiles)), dim3(kIbBlock), 0, s, hist, a.g, ib::clip_count(p.clip_limit, a.g.total),
                         lut);
    }
    if (run.out_lut) PCP_HIP_TRY(ctx, hipMemcpyAsync(run.out_lut, lut, static_cast<size_t>(tiles) * ib::kBins, hipMemcpyDeviceToHost, s));
  }
  {
    BalanceTimed t(ctx, run.timed);
    if ((w & 3) == 0)
      hipLaunchKernelGGL(k_balance_apply<4>, dim3(static_cast<uint32_t>(div_up(w, kIbBlock * 4)), static_cast<uint32_t>(h)), dim3(kIbBlock), 0, s,
                         texels, a, lut, gamma, run.hsv_tables);
    else
      hipLaunchKernelGGL(k_balance_apply<1>, dim3(static_cast<uint32_t>(div_up(w, kIbBlock)), static_cast<uint32_t>(h)), dim3(kIbBlock), 0, s,
                         texels, a, lut, gamma, run.hsv_tables);
  }
  PCP_HIP_TRY(ctx, hipGetLastError());
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

void pcp_default_balance_params(pcp_balance_params *p) {
  if (!p) return;
  p->stages = PCP_BALANCE_CLAHE | PCP_BALANCE_GAMMA;
  p->tiles_x = p->tiles_y = 8;
  p->clip_limit = 1.0f;
  p->gamma = 0.8f;
}

int pcp_gamma_table_host(float gamma, uint8_t out[256]) {
  if (!out || !std::isfinite(gamma) || !(gamma > 0.0f)) {
    set_global_error("pcp_gamma_table_host: NULL table or a gamma that is not finite and > 0");
    return PCP_ERR_INVALID;
  }
  ib::gamma_table(gamma, out);
  return PCP_OK;
}

int pcp_set_image_balance(pcp_context *ctx, const pcp_balance_params *params) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!params || params->stages == 0) {
    ctx->balance = pcp_balance_params{};
    return PCP_OK;
  }
  if (const char *why = balance_params_fault(params)) return set_error(ctx, PCP_ERR_INVALID, "pcp_set_image_balance: %s", why);
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = ensure_hsv_tables(ctx);
  if (rc != PCP_OK) return rc;
  // uploads in flight may still be reading the table of the previous setting from this context
  for (hipStream_t us : ctx->upload_stream)
    if (us) PCP_HIP_TRY(ctx, hipStreamSynchronize(us));
  ib::gamma_table(params->gamma, ctx->balance_gamma);
  ctx->balance = *params;
  ++ctx->balance_seq;
  return PCP_OK;
}

int pcp_image_balance_host(const pcp_balance_params *params, int32_t w, int32_t h, const uint8_t *bgr, int64_t row_stride_bytes,
                           uint8_t *out_bgr, uint32_t *out_hist, uint8_t *out_lut) {
  if (!params || !bgr || w < 1 || h < 1 || row_stride_bytes < 3 * static_cast<int64_t>(w)) {
    set_global_error("pcp_image_balance_host: NULL params or image, an empty image or a row stride < 3*width");
    return PCP_ERR_INVALID;
  }
  if (const char *why = balance_params_fault(params)) {
    set_global_error("pcp_image_balance_host: %s", why);
    return PCP_ERR_INVALID;
  }
  if (w > kIbMaxSide || h > kIbMaxSide || static_cast<int64_t>(w) * h > kIbMaxPixels) {
    set_global_error("pcp_image_balance_host: %d x %d pixels: a side above %d or more than 2^26 pixels", w, h, kIbMaxSide);
    return PCP_ERR_RANGE;
  }
  const bool clahe = params->stages & PCP_BALANCE_CLAHE, gam = params->stages & PCP_BALANCE_GAMMA;
  ib::Grid g{};
  if (clahe && ib::make_grid(w, h, params->tiles_x, params->tiles_y, &g) != 0) {
    set_global_error("pcp_image_balance_host: a %d x %d image cannot be extended to %d x %d tiles by reflection (IB3)", w, h, params->tiles_x,
                     params->tiles_y);
    return PCP_ERR_RANGE;
  }
  int32_t sdiv[256], hdiv[256];
  hsv_build_tables(sdiv, hdiv);
  uint8_t gamma[256];
  ib::gamma_table(params->gamma, gamma);
  std::vector<uint8_t> lut;
  if (clahe) {
    const int32_t tiles = g.tiles_x * g.tiles_y, clip = ib::clip_count(params->clip_limit, g.total);
    lut.resize(static_cast<size_t>(tiles) * ib::kBins);
    for (int32_t tile = 0; tile < tiles; ++tile) {
      const int32_t ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
      int32_t hist[ib::kBins] = {};
      for (int32_t p = 0; p < g.total; ++p) {
        const int32_t row = p / g.tw, col = p - row * g.tw;
        const uint8_t *px = bgr + static_cast<int64_t>(ib::reflect101(ty * g.th + row, h)) * row_stride_bytes + 3 * ib::reflect101(tx * g.tw + col, w);
        ++hist[std::max(px[0], std::max(px[1], px[2]))];
      }
      if (out_hist)
        for (int i = 0; i < ib::kBins; ++i) out_hist[static_cast<size_t>(tile) * ib::kBins + i] = static_cast<uint32_t>(hist[i]);
      int32_t clipped = 0;
      for (int i = 0; i < ib::kBins; ++i) clipped += ib::excess(hist[i], clip);
      int32_t cum = 0;
      for (int i = 0; i < ib::kBins; ++i) {
        cum += ib::redistributed(hist[i], i, clip, clipped);
        lut[static_cast<size_t>(tile) * ib::kBins + i] = static_cast<uint8_t>(ib::lut_entry(cum, g.lut_scale));
      }
    }
    if (out_lut) std::copy(lut.begin(), lut.end(), out_lut);
  }
  if (!out_bgr) return PCP_OK;
  for (int32_t y = 0; y < h; ++y) {
    const ib::Weights wy = clahe ? ib::weights(y, g.inv_th, g.tiles_y) : ib::Weights{};
    const uint8_t *in = bgr + static_cast<int64_t>(y) * row_stride_bytes;
    uint8_t *out = out_bgr + static_cast<int64_t>(y) * 3 * w;
    for (int32_t x = 0; x < w; ++x) {
      uint32_t b = in[3 * x], gg = in[3 * x + 1], r = in[3 * x + 2];
      if (clahe) {
        uint32_t H, S, V;
        hsv_forward(sdiv, hdiv, b, gg, r, H, S, V);
        const ib::Weights wx = ib::weights(x, g.inv_tw, g.tiles_x);
        hsv_backward(H, S, ib::lookup4(lut.data(), g.tiles_x, wx, wy, V), b, gg, r);
      }
      if (gam) {
        b = gamma[b];
        gg = gamma[gg];
        r = gamma[r];
      }
      out[3 * x] = static_cast<uint8_t>(b);
      out[3 * x + 1] = static_cast<uint8_t>(gg);
      out[3 * x + 2] = static_cast<uint8_t>(r);
    }
  }
  return PCP_OK;
}

int pcp_image_balance(pcp_context *ctx, const pcp_balance_params *params, int32_t w, int32_t h, const uint8_t *bgr,
                      int64_t row_stride_bytes, uint8_t *out_bgr, uint32_t *out_hist, uint8_t *out_lut) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!params || !bgr || w < 1 || h < 1 || row_stride_bytes < 3 * static_cast<int64_t>(w))
    return set_error(ctx, PCP_ERR_INVALID, "pcp_image_balance: NULL params or image, an empty image or a row stride < 3*width");
  if (const char *why = balance_params_fault(params)) return set_error(ctx, PCP_ERR_INVALID, "pcp_image_balance: %s", why);
  if (w > kIbMaxSide || h > kIbMaxSide || static_cast<int64_t>(w) * h > kIbMaxPixels)
    return set_error(ctx, PCP_ERR_RANGE, "pcp_image_balance: %d x %d pixels: a side above %d or more than 2^26 pixels", w, h, kIbMaxSide);
  int rc = balance_check(ctx, "pcp_image_balance", *params, w, h);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if ((rc = ensure_hsv_tables(ctx)) != PCP_OK) return rc;
  // lane 0's scratch, on the context's stream: uploads in flight on the lanes finish first
  for (hipStream_t us : ctx->upload_stream)
    if (us) PCP_HIP_TRY(ctx, hipStreamSynchronize(us));
  hipStream_t s = ctx->stream;
  if ((rc = balance_scratch(ctx, 0, s)) != PCP_OK) return rc;
  const int64_t px = static_cast<int64_t>(w) * h;
  PCP_HIP_TRY(ctx, ctx->balance_image.ensure(static_cast<size_t>(px) + 4));
  PCP_HIP_TRY(ctx, ctx->balance_bytes.ensure(static_cast<size_t>(3 * px) + 16));
  PCP_HIP_TRY(ctx, hipMemcpy2DAsync(ctx->balance_bytes.p, static_cast<size_t>(3) * w, bgr, static_cast<size_t>(row_stride_bytes),
                                    static_cast<size_t>(3) * w, static_cast<size_t>(h), hipMemcpyHostToDevice, s));
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    pack_bgr_texels(s, ctx->balance_bytes.p, 3 * static_cast<int64_t>(w), w, h, ctx->balance_image.p, 1, nullptr, 1.0f, 1.0f);
  }
  uint8_t gamma[256];
  ib::gamma_table(params->gamma, gamma);
  BalanceRun run{};
  run.params = *params;
  run.gamma_host = gamma;
  run.gamma_stale = true;
  ctx->balance_lane_seq[0] = 0;  // the lane's copy of the setting's table is gone
  run.hsv_tables = ctx->hsv_tables.p;
  run.timed = true;
  run.out_hist = out_hist;
  run.out_lut = out_lut;
  if ((rc = balance_texels(ctx, 0, s, run, w, h, ctx->balance_image.p)) != PCP_OK) {
    (void)hipStreamSynchronize(s);  // `gamma` lives on this stack frame
    return rc;
  }
  if (out_bgr) {
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_balance_unpack, dim3(static_cast<uint32_t>(div_up(px, kIbBlock))), dim3(kIbBlock), 0, s, ctx->balance_image.p, px,
                         ctx->balance_bytes.p);
    }
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_bgr, ctx->balance_bytes.p, static_cast<size_t>(3 * px), hipMemcpyDeviceToHost, s));
  }
  const hipError_t e = hipStreamSynchronize(s);
  PCP_HIP_TRY(ctx, e);
  return drain_timing(ctx);
}

}  // extern "C"
