// pcp_mask_edt.hip -- mask distance maps ("Mask distance maps"): the exact squared Euclidean distance from every
// pixel of a keyframe's mask to the nearest background pixel, and that pixel's linear index -- what
// scripts/genNormAndDistanceMask.py preprocess() :150-198 gets from cv2.threshold :167 and
// scipy.ndimage.distance_transform_edt :168 on the host.  The mask is the top byte of the keyframe's texel
// (pcp_upload_mask), so nothing is uploaded.  Separable: a column stage (vertical distance and row of the nearest
// background pixel of the pixel's own column, ties to the upper row) and a row stage (the smallest 64-bit key
// d2 << 32 | index over the columns of the pixel's row).  The per-element arithmetic is pcp_mask_edt.hpp's, shared with
// pcp_mask_edt_host.  Every loop is bounded by the image size for any mask; there are no atomics.
#include <algorithm>
#include <new>
#include <thread>

#include "pcp_internal.hpp"
#include "pcp_mask_edt.hpp"

namespace pcp {

constexpr int kMdBlock = 256;
// keyframes per launch of the batched form: as many as fit this many pixels (12 B of device memory per pixel)
constexpr int64_t kMdChunkPixels = int64_t(1) << 26;

// ---- column stage -------------------------------------------------------------------------------------------------
// One lane per (column, segment of 64 rows, keyframe): consecutive lanes take consecutive x, so every row of the segment is
// one coalesced read.  Bit j of the word = pixel (x, 64 * s + j) is background; rows past the image stay 0.
__global__ __launch_bounds__(kMdBlock) void k_md_bits(const uint32_t *__restrict__ texels, int32_t w, int32_t h, int32_t segs,
                                                      int32_t threshold, unsigned long long *__restrict__ bits) {
  const int32_t x = static_cast<int32_t>(blockIdx.x) * kMdBlock + static_cast<int32_t>(threadIdx.x);
  if (x >= w) return;
  const int32_t s = static_cast<int32_t>(blockIdx.y), f = static_cast<int32_t>(blockIdx.z);
  const uint32_t *img = texels + static_cast<int64_t>(f) * w * h;
  const int32_t y0 = s * md::kSegmentRows, y1 = min(h, y0 + md::kSegmentRows);
  unsigned long long m = 0;
  for (int32_t y = y0; y < y1; ++y)
    if (!md::foreground(img[static_cast<int64_t>(y) * w + x] >> 24, threshold)) m |= 1ull << (y - y0);
  bits[(static_cast<int64_t>(f) * segs + s) * w + x] = m;
}

// The same lanes: the nearest background row above the segment and below it from the other segments' words (the carried
// boundary: at most `segs` words each way), then the column word of each of the segment's pixels from its own word.
__global__ __launch_bounds__(kMdBlock) void k_md_columns(const unsigned long long *__restrict__ bits, int32_t w, int32_t h,
                                                         int32_t segs, uint32_t *__restrict__ col) {
  const int32_t x = static_cast<int32_t>(blockIdx.x) * kMdBlock + static_cast<int32_t>(threadIdx.x);
  if (x >= w) return;
  const int32_t s = static_cast<int32_t>(blockIdx.y), f = static_cast<int32_t>(blockIdx.z);
  const unsigned long long *fb = bits + static_cast<int64_t>(f) * segs * w + x;
  const unsigned long long m = fb[static_cast<int64_t>(s) * w];
  int32_t above = -1, below = -1;
  for (int32_t sp = s - 1; sp >= 0; --sp) {
    const unsigned long long mm = fb[static_cast<int64_t>(sp) * w];
    if (mm) {
      above = sp * md::kSegmentRows + 63 - __clzll(static_cast<long long>(mm));
      break;
    }
  }
  for (int32_t sp = s + 1; sp < segs; ++sp) {
    const unsigned long long mm = fb[static_cast<int64_t>(sp) * w];
    if (mm) {
      below = sp * md::kSegmentRows + __ffsll(mm) - 1;
      break;
    }
  }
  const int32_t y0 = s * md::kSegmentRows, y1 = min(h, y0 + md::kSegmentRows);
  uint32_t *out = col + static_cast<int64_t>(f) * w * h + x;
  for (int32_t y = y0; y < y1; ++y) {
    const int32_t j = y - y0;
    const unsigned long long lo = m & (~0ull >> (63 - j)), hi = m & (~0ull << j);  // bits 0..j, bits j..63
    const int32_t up = lo ? y0 + 63 - __clzll(static_cast<long long>(lo)) : above;
    const int32_t down = hi ? y0 + __ffsll(hi) - 1 : below;
    out[static_cast<int64_t>(y) * w] = md::column_word(y, md::column_pick(y, up, down));
  }
}

// ---- row stage ----------------------------------------------------------------------------------------------------
// One workgroup per (row, keyframe): the row's column words in LDS (4 B per pixel, 64 KB at the widest image), then every
// lane searches outward from its own pixel (md::row_search) -- neighbouring lanes read neighbouring words.
__global__ __launch_bounds__(kMdBlock) void k_md_rows(const uint32_t *__restrict__ col, int32_t w, int32_t h,
                                                      uint32_t *__restrict__ out_d2, int32_t *__restrict__ out_nearest) {
  extern __shared__ uint32_t s_row[];
  const int64_t base = (static_cast<int64_t>(blockIdx.y) * h + static_cast<int64_t>(blockIdx.x)) * w;
  for (int32_t x = static_cast<int32_t>(threadIdx.x); x < w; x += kMdBlock) s_row[x] = col[base + x];
  __syncthreads();
  for (int32_t x = static_cast<int32_t>(threadIdx.x); x < w; x += kMdBlock) {
    const unsigned long long key = md::row_search(s_row, x, w);
    out_d2[base + x] = md::key_d2(key);
    if (out_nearest) out_nearest[base + x] = md::key_nearest(key);
  }
}

hipError_t preload_mask_edt() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_md_rows));
}

// device memory for `chunk` keyframes per launch
static int mask_edt_reserve(pcp_context *ctx, int32_t chunk, bool want_nearest) {
  const int32_t w = ctx->dcam.img_w, h = ctx->dcam.img_h;
  const int32_t segs = (h + md::kSegmentRows - 1) / md::kSegmentRows;
  const size_t cpx = static_cast<size_t>(chunk) * static_cast<size_t>(w) * static_cast<size_t>(h);
  PCP_HIP_TRY(ctx, ctx->md_bits.ensure(static_cast<size_t>(chunk) * segs * w + 4));
  PCP_HIP_TRY(ctx, ctx->md_col.ensure(cpx + 4));
  PCP_HIP_TRY(ctx, ctx->md_d2.ensure(cpx + 4));
  if (want_nearest) PCP_HIP_TRY(ctx, ctx->md_nearest.ensure(cpx + 4));
  return PCP_OK;
}

// the three launches of keyframes [first, first + nf) of one chunk: their results stay in md_bits / md_d2 / md_nearest
static int mask_edt_launch(pcp_context *ctx, int32_t first, int32_t nf, int32_t threshold, bool want_nearest) {
  const int32_t w = ctx->dcam.img_w, h = ctx->dcam.img_h;
  const int64_t px = static_cast<int64_t>(w) * h;
  const int32_t segs = (h + md::kSegmentRows - 1) / md::kSegmentRows;
  const dim3 cgrid(static_cast<uint32_t>((w + kMdBlock - 1) / kMdBlock), static_cast<uint32_t>(segs), static_cast<uint32_t>(nf));
  const uint32_t *texels = ctx->images.p + static_cast<int64_t>(first) * px;
  {
    LaunchTimer lt(ctx, PCP_K_MISC);  // column stage
    hipLaunchKernelGGL(k_md_bits, cgrid, dim3(kMdBlock), 0, ctx->stream, texels, w, h, segs, threshold, ctx->md_bits.p);
    hipLaunchKernelGGL(k_md_columns, cgrid, dim3(kMdBlock), 0, ctx->stream, ctx->md_bits.p, w, h, segs, ctx->md_col.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer lt(ctx, PCP_K_MISC);  // row stage
    hipLaunchKernelGGL(k_md_rows, dim3(static_cast<uint32_t>(h), static_cast<uint32_t>(nf)), dim3(kMdBlock),
                       static_cast<size_t>(w) * sizeof(uint32_t), ctx->stream, ctx->md_col.p, w, h, ctx->md_d2.p,
                       want_nearest ? ctx->md_nearest.p : static_cast<int32_t *>(nullptr));
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return PCP_OK;
}

// keyframes [first, first + count) of a checked call: chunks of keyframes, three launches each, the images of a chunk copied
// to the host behind its kernels
static int mask_edt_run(pcp_context *ctx, int32_t first, int32_t count, int32_t threshold, uint32_t *out_d2, int32_t *out_nearest) {
  const int64_t px = static_cast<int64_t>(ctx->dcam.img_w) * ctx->dcam.img_h;
  const int32_t chunk = static_cast<int32_t>(std::min<int64_t>({count, std::max<int64_t>(1, kMdChunkPixels / px), 65535}));
  int rc = mask_edt_reserve(ctx, chunk, out_nearest != nullptr);
  if (rc != PCP_OK) return rc;
  if ((rc = wait_images(ctx, first, first + count)) != PCP_OK) return rc;  // the mask byte shares its word with the colour
  for (int32_t f0 = 0; f0 < count; f0 += chunk) {
    const int32_t nf = std::min(chunk, count - f0);
    if ((rc = mask_edt_launch(ctx, first + f0, nf, threshold, out_nearest != nullptr)) != PCP_OK) return rc;
    const size_t words = static_cast<size_t>(nf) * static_cast<size_t>(px), at = static_cast<size_t>(f0) * static_cast<size_t>(px);
    if (out_d2) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_d2 + at, ctx->md_d2.p, words * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_nearest) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_nearest + at, ctx->md_nearest.p, words * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

// what every call checks before it touches the device
static int mask_edt_validate(pcp_context *ctx, const char *who, int32_t first, int32_t count, int32_t threshold) {
  if (!ctx) return PCP_ERR_INVALID;
  if (threshold < 0 || threshold > 255) return set_error(ctx, PCP_ERR_INVALID, "%s: threshold %d outside 0..255", who, threshold);
  if (!ctx->have_camera) return set_error(ctx, PCP_ERR_STATE, "%s: pcp_set_camera has not been called", who);
  if (ctx->n_frames <= 0) return set_error(ctx, PCP_ERR_STATE, "%s: pcp_set_frames has not been called", who);
  if (count < 0 || first < 0 || first >= ctx->n_frames || count > ctx->n_frames - first)
    return set_error(ctx, PCP_ERR_RANGE, "%s: keyframes [%d, %d) outside 0..%d", who, first, first + count, ctx->n_frames);
  const int32_t w = ctx->dcam.img_w, h = ctx->dcam.img_h;
  if (w > md::kMaxSide || h > md::kMaxSide)
    return set_error(ctx, PCP_ERR_RANGE, "%s: image %d x %d exceeds %d a side", who, w, h, md::kMaxSide);
  for (int32_t f = first; f < first + count; ++f)
    if (!ctx->images.p || static_cast<size_t>(f) >= ctx->mask_set.size() || !ctx->mask_set[static_cast<size_t>(f)])
      return set_error(ctx, PCP_ERR_STATE, "%s: no mask uploaded for keyframe %d (pcp_upload_mask)", who, f);
  return PCP_OK;
}

static int mask_edt_checked(pcp_context *ctx, const char *who, int32_t first, int32_t count, int32_t threshold, uint32_t *out_d2,
                            int32_t *out_nearest) {
  const int rc = mask_edt_validate(ctx, who, first, count, threshold);
  if (rc != PCP_OK) return rc;
  if (count == 0 || ctx->dcam.img_w <= 0 || ctx->dcam.img_h <= 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  return mask_edt_run(ctx, first, count, threshold, out_d2, out_nearest);
}

// The device part of pcp_mask_edt for one keyframe, for the stages that read the maps where they are (pcp_crack_width.hip):
// checks under the caller's name, then the kernels; background bits, d2 and nearest of the keyframe stay in md_bits, md_d2
// and md_nearest.  Nothing is copied and the stream is not synchronised.  The image must not be empty.
int mask_edt_device(pcp_context *ctx, const char *who, int32_t frame, int32_t threshold) {
  int rc = mask_edt_validate(ctx, who, frame, 1, threshold);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if ((rc = mask_edt_reserve(ctx, 1, true)) != PCP_OK) return rc;
  if ((rc = wait_images(ctx, frame, frame + 1)) != PCP_OK) return rc;
  return mask_edt_launch(ctx, frame, 1, threshold, true);
}

// the column and row stages on a bit image that another stage built (pcp_internal.hpp)
int mask_edt_of_bits(pcp_context *ctx, const unsigned long long *bits, int32_t w, int32_t h, int32_t segs, uint32_t *col,
                     uint32_t *out_d2, int32_t *out_nearest) {
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_md_columns, dim3(static_cast<uint32_t>((w + kMdBlock - 1) / kMdBlock), static_cast<uint32_t>(segs), 1u),
                       dim3(kMdBlock), 0, ctx->stream, bits, w, h, segs, col);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_md_rows, dim3(static_cast<uint32_t>(h), 1u), dim3(kMdBlock), static_cast<size_t>(w) * sizeof(uint32_t),
                       ctx->stream, col, w, h, out_d2, out_nearest);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_mask_edt(pcp_context *ctx, int32_t frame, int32_t threshold, uint32_t *out_d2, int32_t *out_nearest) {
  return mask_edt_checked(ctx, "pcp_mask_edt", frame, 1, threshold, out_d2, out_nearest);
}

int pcp_mask_edt_frames(pcp_context *ctx, int32_t first_frame, int32_t count, int32_t threshold, uint32_t *out_d2,
                        int32_t *out_nearest) {
  return mask_edt_checked(ctx, "pcp_mask_edt_frames", first_frame, count, threshold, out_d2, out_nearest);
}

int pcp_mask_edt_host(int32_t width, int32_t height, const uint8_t *gray, int64_t row_stride_bytes, int32_t threshold,
                      uint32_t *out_d2, int32_t *out_nearest) {
  if (width <= 0 || height <= 0 || !gray || row_stride_bytes < static_cast<int64_t>(width)) {
    set_global_error("pcp_mask_edt_host: empty image, NULL mask or row stride < width");
    return PCP_ERR_INVALID;
  }
  if (threshold < 0 || threshold > 255) {
    set_global_error("pcp_mask_edt_host: threshold %d outside 0..255", threshold);
    return PCP_ERR_INVALID;
  }
  if (width > md::kMaxSide || height > md::kMaxSide) {
    set_global_error("pcp_mask_edt_host: image %d x %d exceeds %d a side", width, height, md::kMaxSide);
    return PCP_ERR_RANGE;
  }
  const size_t w = static_cast<size_t>(width), h = static_cast<size_t>(height);
  std::vector<uint32_t> col;
  std::vector<int32_t> up;
  try {
    col.resize(w * h);
    up.resize(h);
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_mask_edt_host: out of host memory for %d x %d pixels", width, height);
    return PCP_ERR_NOMEM;
  }
  // column stage: the nearest background row at or above every pixel going down, at or below it going up
  for (int32_t x = 0; x < width; ++x) {
    int32_t last = -1;
    for (int32_t y = 0; y < height; ++y) {
      if (!md::foreground(gray[static_cast<int64_t>(y) * row_stride_bytes + x], threshold)) last = y;
      up[static_cast<size_t>(y)] = last;
    }
    last = -1;
    for (int32_t y = height - 1; y >= 0; --y) {
      if (!md::foreground(gray[static_cast<int64_t>(y) * row_stride_bytes + x], threshold)) last = y;
      col[static_cast<size_t>(y) * w + static_cast<size_t>(x)] = md::column_word(y, md::column_pick(y, up[static_cast<size_t>(y)], last));
    }
  }
  // row stage: the rows do not interact, up to 8 host threads share them
  auto rows = [&](int32_t y0, int32_t y1) {
    for (int32_t y = y0; y < y1; ++y) {
      const uint32_t *row = col.data() + static_cast<size_t>(y) * w;
      for (int32_t x = 0; x < width; ++x) {
        const unsigned long long key = md::row_search(row, x, width);
        const size_t at = static_cast<size_t>(y) * w + static_cast<size_t>(x);
        if (out_d2) out_d2[at] = md::key_d2(key);
        if (out_nearest) out_nearest[at] = md::key_nearest(key);
      }
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
