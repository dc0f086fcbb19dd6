// pcp_jpeg.hip -- pcp_upload_image_jpeg: the pixels of a keyframe JPEG reconstructed on the device from the quantised
// coefficients the host's entropy decoder hands over (host/image_io.hpp jpeg_coefficients; blob layout: pcp_jpeg_header,
// include/pcp_hip.h), bit for bit what the host decoder (and libjpeg, which cv::imread links) produces:
//   k_jpeg_idct    dequantisation + jidctint.c's islow IDCT, 32-bit integer arithmetic in the same order, range limit:
//                  each component's plane (blocks_w*8 x blocks_h*8 bytes) in the upload lane's scratch buffer;
//   k_jpeg_pixels  jdsample.c's fullsize / h2v1 / h2v2 "fancy" upsampling (box when down_w <= 2) in closed form per output
//                  pixel, jdcolor.c's YCbCr->RGB tables (grey: B = G = R = Y), then pcp_set_image_adjust's round trip
//                  (pcp_hsv.hpp, the function the BGR pack kernels call) and the texel store with the mask byte rule of
//                  k_pack_bgr.
// The lanes, events and keyframe bookkeeping are pcp_colour.hip's upload_texels, shared with pcp_upload_image.
#include <algorithm>
#include <cstring>

#include "pcp_hsv.hpp"
#include "pcp_internal.hpp"

namespace pcp {

constexpr int kJpegBlock = 256;
constexpr int kJpegBlocksPerGroup = kJpegBlock / 8;  // 8 lanes per 8x8 block

// a validated blob's geometry (jpeg_check)
struct JpegGeom {
  int32_t width, height, ncomp, mcux, per_mcu, hmax, vmax;
  int32_t h[3], v[3], first[3], stride[3], down_w[3], down_h[3];
  int64_t plane_off[3];
  int64_t n_blocks;
};

// jidctint.c constants (CONST_BITS 13, PASS1_BITS 2)
constexpr int32_t kF0298 = 2446, kF0390 = 3196, kF0541 = 4433, kF0765 = 6270, kF0899 = 7373, kF1175 = 9633, kF1501 = 12299,
                  kF1847 = 15137, kF1961 = 16069, kF2053 = 16819, kF2562 = 20995, kF3072 = 25172;

// one 1-D islow pass over x[0..7] (even part from x0 x2 x4 x6, odd part from x1 x3 x5 x7), before descaling, in output order
__device__ __forceinline__ void islow_pass(const int32_t x[8], int32_t o[8]) {
  int32_t z2 = x[2], z3 = x[6];
  int32_t z1 = (z2 + z3) * kF0541;
  int32_t tmp2 = z1 + z3 * (-kF1847), tmp3 = z1 + z2 * kF0765;
  int32_t tmp0 = (x[0] + x[4]) * (1 << 13), tmp1 = (x[0] - x[4]) * (1 << 13);
  const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = x[7];
  tmp1 = x[5];
  tmp2 = x[3];
  tmp3 = x[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int32_t z4 = tmp1 + tmp3;
  const int32_t z5 = (z3 + z4) * kF1175;
  tmp0 *= kF0298;
  tmp1 *= kF2053;
  tmp2 *= kF3072;
  tmp3 *= kF1501;
  z1 *= -kF0899;
  z2 *= -kF2562;
  z3 *= -kF1961;
  z4 *= -kF0390;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  o[0] = tmp10 + tmp3;
  o[7] = tmp10 - tmp3;
  o[1] = tmp11 + tmp2;
  o[6] = tmp11 - tmp2;
  o[2] = tmp12 + tmp1;
  o[5] = tmp12 - tmp1;
  o[3] = tmp13 + tmp0;
  o[4] = tmp13 - tmp0;
}

__device__ __forceinline__ int32_t descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ uint32_t clamp8(int32_t v) { return static_cast<uint32_t>(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// 8 lanes per block, 8 blocks per wavefront.  Lane c: column c (its coefficients expanded from the mask, dequantised,
// column pass) -> LDS -> row c (row pass, +128, clamp) -> one 8-byte store into the component's plane.
__global__ __launch_bounds__(kJpegBlock) void k_jpeg_idct(const uint64_t *__restrict__ masks, const uint32_t *__restrict__ offsets,
                                                          const int16_t *__restrict__ values, const uint16_t *__restrict__ quant,
                                                          JpegGeom g, uint8_t *__restrict__ planes) {
  __shared__ int32_t ws[kJpegBlocksPerGroup * 64];
  const int lb = threadIdx.x >> 3, c = threadIdx.x & 7;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kJpegBlocksPerGroup + lb;
  const bool live = b < g.n_blocks;
  int comp = 0;
  int64_t row0 = 0, col0 = 0;
  if (live) {
    // position from the decode order: MCU row, MCU, component, v, h
    const int64_t m = b / g.per_mcu;
    const int r = static_cast<int>(b - m * g.per_mcu);
    comp = g.ncomp == 3 ? (r >= g.first[2] ? 2 : (r >= g.first[1] ? 1 : 0)) : 0;
    const int rr = r - g.first[comp], by = rr / g.h[comp], bx = rr - by * g.h[comp];
    const int64_t my = m / g.mcux, mx = m - my * g.mcux;
    row0 = (my * g.v[comp] + by) * 8;
    col0 = (mx * g.h[comp] + bx) * 8;
    const uint64_t mask = masks[b];
    const int64_t off = offsets[b];
    const uint16_t *q = quant + comp * 64;
    int32_t x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int n = 8 * k + c;
      const bool nz = (mask >> n) & 1u;
      const int32_t idx = __popcll(mask & ((uint64_t(1) << n) - 1));
      x[k] = nz ? static_cast<int32_t>(values[off + idx]) * static_cast<int32_t>(q[n]) : 0;
    }
    int32_t *w = ws + lb * 64 + c;
    if ((mask & (0x0101010101010100ull << c)) == 0) {  // the DC-only column shortcut of jidctint.c (exact)
      const int32_t dcv = x[0] * (1 << 2);
#pragma unroll
      for (int k = 0; k < 8; ++k) w[8 * k] = dcv;
    } else {
      int32_t o[8];
      islow_pass(x, o);
#pragma unroll
      for (int k = 0; k < 8; ++k) w[8 * k] = descale(o[k], 13 - 2);
    }
  }
  __syncthreads();
  if (!live) return;
  int32_t x[8], o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = ws[lb * 64 + 8 * c + k];
  islow_pass(x, o);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lo |= clamp8(descale(o[k], 13 + 2 + 3) + 128) << (8 * k);
    hi |= clamp8(descale(o[k + 4], 13 + 2 + 3) + 128) << (8 * k);
  }
  uint8_t *dst = planes + g.plane_off[comp] + (row0 + c) * g.stride[comp] + col0;
  *reinterpret_cast<uint2 *>(dst) = make_uint2(lo, hi);
}

// one upsampled sample of component `c` at output pixel (x, y): jdsample.c in closed form (host/image_io.hpp upsample)
__device__ __forceinline__ int32_t jpeg_sample(const uint8_t *__restrict__ planes, const JpegGeom &g, int c, int32_t x, int32_t y) {
  const uint8_t *p = planes + g.plane_off[c];
  const int64_t s = g.stride[c];
  if (g.h[c] == g.hmax && g.v[c] == g.vmax) return p[y * s + x];
  const int32_t dw = g.down_w[c], i = x >> 1;
  const bool odd = x & 1;
  if (g.v[c] == g.vmax) {  // h2v1
    const uint8_t *in = p + y * s;
    if (dw <= 2) return in[i];
    if (!odd) return i == 0 ? in[0] : (in[i] * 3 + in[i - 1] + 1) >> 2;
    return i == dw - 1 ? in[dw - 1] : (in[i] * 3 + in[i + 1] + 2) >> 2;
  }
  // h2v2: the nearer input row weighs 3, the other (replicated at the edges) 1; then the same across columns
  const int32_t r = y >> 1;
  const uint8_t *in0 = p + r * s;
  if (dw <= 2) return in0[i];
  const int32_t rn = (y & 1) == 0 ? (r > 0 ? r - 1 : 0) : (r + 1 < g.down_h[c] ? r + 1 : g.down_h[c] - 1);
  const uint8_t *in1 = p + rn * s;
  const int32_t cur = in0[i] * 3 + in1[i];
  if (!odd) {
    if (i == 0) return (cur * 4 + 8) >> 4;
    return (cur * 3 + in0[i - 1] * 3 + in1[i - 1] + 8) >> 4;
  }
  if (i == dw - 1) return (cur * 4 + 7) >> 4;
  return (cur * 3 + in0[i + 1] * 3 + in1[i + 1] + 7) >> 4;
}

__global__ __launch_bounds__(kJpegBlock) void k_jpeg_pixels(const uint8_t *__restrict__ planes, JpegGeom g,
                                                            uint32_t *__restrict__ texels, int32_t clear_mask,
                                                            const int32_t *__restrict__ hsv_tables, float sat_scale,
                                                            float val_scale) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kJpegBlock + threadIdx.x;
  if (i >= static_cast<int64_t>(g.width) * g.height) return;
  const int32_t y = static_cast<int32_t>(i / g.width), x = static_cast<int32_t>(i - static_cast<int64_t>(y) * g.width);
  const int32_t Y = jpeg_sample(planes, g, 0, x, y);
  uint32_t b, gg, r;
  if (g.ncomp == 1) {
    b = gg = r = static_cast<uint32_t>(Y);
  } else {
    // jdcolor.c build_ycc_rgb_table, SCALEBITS 16: the table entries computed in place
    const int32_t cb = jpeg_sample(planes, g, 1, x, y) - 128, cr = jpeg_sample(planes, g, 2, x, y) - 128;
    r = clamp8(Y + ((91881 * cr + 32768) >> 16));                   // FIX(1.40200)
    gg = clamp8(Y + ((-22554 * cb + 32768 + -46802 * cr) >> 16));   // -FIX(0.34414) + ONE_HALF, -FIX(0.71414)
    b = clamp8(Y + ((116130 * cb + 32768) >> 16));                  // FIX(1.77200)
  }
  if (hsv_tables) hsv_round_trip(hsv_tables, hsv_tables + 256, sat_scale, val_scale, b, gg, r);
  const uint32_t keep = clear_mask ? 0u : (texels[i] & 0xff000000u);
  texels[i] = keep | b | (gg << 8) | (r << 16);
}

hipError_t preload_jpeg() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_jpeg_idct));
}

// The blob, checked on the host before anything is queued: a malformed one (it comes from a file) must never make the
// kernels read or write out of bounds.
struct JpegSource final : TexelSource {
  const uint8_t *blob;
  int64_t bytes;
  pcp_jpeg_header hd{};
  JpegGeom g{};
  int64_t used = 0, plane_bytes = 0;
  const uint8_t *dev = nullptr;
  JpegSource(const uint8_t *b, int64_t n) : blob(b), bytes(n) {}

  int validate(pcp_context *ctx, const char *who) override {
    if (!blob || bytes < static_cast<int64_t>(sizeof(pcp_jpeg_header)))
      return set_error(ctx, PCP_ERR_INVALID, "%s: NULL blob or fewer bytes (%lld) than its header", who, static_cast<long long>(bytes));
    std::memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != PCP_JPEG_MAGIC || hd.version != PCP_JPEG_VERSION)
      return set_error(ctx, PCP_ERR_INVALID, "%s: not a coefficient blob of version %d (magic 0x%08x, version %u)", who,
                       PCP_JPEG_VERSION, hd.magic, hd.version);
    if (hd.width != ctx->dcam.img_w || hd.height != ctx->dcam.img_h)
      return set_error(ctx, PCP_ERR_INVALID, "%s: image %dx%d, the camera's is %dx%d", who, hd.width, hd.height,
                       ctx->dcam.img_w, ctx->dcam.img_h);
    if (hd.ncomp != 1 && hd.ncomp != 3) return set_error(ctx, PCP_ERR_INVALID, "%s: %d components (1 or 3)", who, hd.ncomp);
    const pcp_jpeg_component *c = hd.comp;
    const bool y_ok = (c[0].h == 1 && c[0].v == 1) || (hd.ncomp == 3 && c[0].h == 2 && (c[0].v == 1 || c[0].v == 2));
    const bool chroma_ok = hd.ncomp == 1 || (c[1].h == 1 && c[1].v == 1 && c[2].h == 1 && c[2].v == 1);
    if (!y_ok || !chroma_ok)
      return set_error(ctx, PCP_ERR_INVALID, "%s: unsupported sampling (component 0 %dx%d; 4:4:4, 4:2:2, 4:2:0 or grey)", who,
                       c[0].h, c[0].v);
    g.width = hd.width;
    g.height = hd.height;
    g.ncomp = hd.ncomp;
    g.hmax = c[0].h;
    g.vmax = c[0].v;
    g.mcux = (hd.width + 8 * g.hmax - 1) / (8 * g.hmax);
    const int32_t mcuy = (hd.height + 8 * g.vmax - 1) / (8 * g.vmax);
    g.per_mcu = 0;
    for (int k = 0; k < 3; ++k) {
      const int kk = k < hd.ncomp ? k : 0;  // (unused entries: copies of component 0, never selected)
      g.h[k] = c[kk].h;
      g.v[k] = c[kk].v;
      g.first[k] = k < hd.ncomp ? g.per_mcu : 1 << 30;
      if (k < hd.ncomp) {
        if (c[k].blocks_w != g.mcux * c[k].h || c[k].blocks_h != mcuy * c[k].v ||
            c[k].down_w != (hd.width * c[k].h + g.hmax - 1) / g.hmax || c[k].down_h != (hd.height * c[k].v + g.vmax - 1) / g.vmax)
          return set_error(ctx, PCP_ERR_INVALID, "%s: component %d: blocks %dx%d / samples %dx%d do not match a %dx%d frame", who,
                           k, c[k].blocks_w, c[k].blocks_h, c[k].down_w, c[k].down_h, hd.width, hd.height);
        g.per_mcu += c[k].h * c[k].v;
      }
      g.stride[k] = c[kk].blocks_w * 8;
      g.down_w[k] = c[kk].down_w;
      g.down_h[k] = c[kk].down_h;
      g.plane_off[k] = k < hd.ncomp ? plane_bytes : 0;
      if (k < hd.ncomp) plane_bytes += static_cast<int64_t>(c[k].blocks_w) * 8 * c[k].blocks_h * 8;
    }
    g.n_blocks = static_cast<int64_t>(g.mcux) * mcuy * g.per_mcu;
    auto a16 = [](int64_t v) { return (v + 15) & ~int64_t(15); };
    const int64_t quant_off = static_cast<int64_t>(sizeof(pcp_jpeg_header)), mask_off = a16(quant_off + 128 * hd.ncomp),
                  offset_off = a16(mask_off + 8 * g.n_blocks), value_off = a16(offset_off + 4 * g.n_blocks);
    if (hd.n_blocks != g.n_blocks || hd.quant_off != quant_off || hd.mask_off != mask_off || hd.offset_off != offset_off ||
        hd.value_off != value_off || hd.n_values < 0 || hd.n_values > 64 * g.n_blocks)
      return set_error(ctx, PCP_ERR_INVALID, "%s: section layout does not match %lld blocks", who, static_cast<long long>(g.n_blocks));
    used = value_off + 2 * hd.n_values;
    if (used > bytes)
      return set_error(ctx, PCP_ERR_INVALID, "%s: truncated blob (%lld bytes, its sections need %lld)", who,
                       static_cast<long long>(bytes), static_cast<long long>(used));
    int64_t expect = 0;
    for (int64_t k = 0; k < g.n_blocks; ++k) {
      uint64_t m;
      uint32_t o;
      std::memcpy(&m, blob + mask_off + 8 * k, 8);
      std::memcpy(&o, blob + offset_off + 4 * k, 4);
      if (o != expect)
        return set_error(ctx, PCP_ERR_INVALID, "%s: block %lld: value offset %u, its predecessors' masks give %lld", who,
                         static_cast<long long>(k), o, static_cast<long long>(expect));
      expect += __builtin_popcountll(m);
    }
    if (expect != hd.n_values)
      return set_error(ctx, PCP_ERR_INVALID, "%s: the masks hold %lld values, the header %lld", who, static_cast<long long>(expect),
                       static_cast<long long>(hd.n_values));
    return PCP_OK;
  }
  int stage(pcp_context *ctx, int lane, hipStream_t us) override {
    PCP_HIP_TRY(ctx, ctx->upload_stage[lane].ensure(static_cast<size_t>(used) + 16));
    PCP_HIP_TRY(ctx, ctx->jpeg_planes[lane].ensure(static_cast<size_t>(plane_bytes)));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(ctx->upload_stage[lane].p, blob, static_cast<size_t>(used), hipMemcpyHostToDevice, us));
    dev = ctx->upload_stage[lane].p;
    return PCP_OK;
  }
  int pack(pcp_context *ctx, int lane, hipStream_t us, int32_t, uint32_t *dst, int32_t clear_mask, const int32_t *tables) override {
    uint8_t *planes = ctx->jpeg_planes[lane].p;
    const uint32_t groups = static_cast<uint32_t>(std::max<int64_t>(1, div_up(g.n_blocks, kJpegBlocksPerGroup)));
    hipLaunchKernelGGL(k_jpeg_idct, dim3(groups), dim3(kJpegBlock), 0, us, reinterpret_cast<const uint64_t *>(dev + hd.mask_off),
                       reinterpret_cast<const uint32_t *>(dev + hd.offset_off), reinterpret_cast<const int16_t *>(dev + hd.value_off),
                       reinterpret_cast<const uint16_t *>(dev + hd.quant_off), g, planes);
    const int64_t px = static_cast<int64_t>(g.width) * g.height;
    hipLaunchKernelGGL(k_jpeg_pixels, dim3(static_cast<uint32_t>(std::max<int64_t>(1, div_up(px, kJpegBlock)))), dim3(kJpegBlock), 0,
                       us, planes, g, dst, clear_mask, tables, ctx->saturation_scale, ctx->brightness_scale);
    return PCP_OK;
  }
};

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_upload_image_jpeg(pcp_context *ctx, int32_t frame, const uint8_t *blob, int64_t bytes) {
  JpegSource source(blob, bytes);
  return upload_texels(ctx, "pcp_upload_image_jpeg", frame, 1, false, true, source);
}

int pcp_upload_image_jpeg_async(pcp_context *ctx, int32_t frame, const uint8_t *blob, int64_t bytes) {
  JpegSource source(blob, bytes);
  return upload_texels(ctx, "pcp_upload_image_jpeg_async", frame, 1, false, false, source);
}

}  // extern "C"
