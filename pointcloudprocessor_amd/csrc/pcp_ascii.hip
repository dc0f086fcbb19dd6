// pcp_ascii.hip -- PCD ASCII rows formatted on the device ("Device PCD writer"): the text of the four writers'
// layouts (host/pcd_io.hpp writeASCII_*), byte for byte, from rows that are already on the device, downloaded as bytes
// that go straight to write().  Opt-in: nothing here runs unless one of the pcp_ascii_* / *_ascii entry points is called.
//
// Three launches per call plus one per window of text:
//   k_ascii_len    a row per lane, a tile of 256 rows per workgroup: the row's length (1 B per row) and the tile's bytes;
//   k_ascii_scan   ONE workgroup: exclusive prefix of the tile bytes in 64 bits (2^28 rows are more than 2^32 bytes),
//                  1024 tiles per round with the carry in a register; entry [tiles] = the total;
//   k_ascii_pick   the prefix at the window boundaries (the host learns each window's byte range and the total from them);
//   k_ascii_emit   per window: a tile per workgroup; the lanes scan their lengths, format their rows into LDS at those
//                  offsets, and the workgroup's contiguous byte range leaves as 16-byte stores from the first 16-byte
//                  boundary of the destination, byte stores only for the unaligned head and tail.
// The text is a pure function of the rows: lengths and bytes come from the same decode (pcp_ascii.hpp).
#include <algorithm>
#include <vector>

#include "pcp_ascii.hpp"
#include "pcp_internal.hpp"

namespace pcp {

constexpr int kAsBlock = 256;         // lanes = rows of a tile
constexpr int kAsScanBlock = 1024;    // tiles per round of the single-workgroup scan
constexpr int kAsMaxRow = 105;        // PCP_ROWS_POINTNORMAL
constexpr int64_t kAsWindowBytes = int64_t(64) << 20;  // device text buffer: a window's rows x the kind's longest row fit

static inline int row_floats(int32_t kind) { return kind == PCP_ROWS_XYZI ? 4 : kind == PCP_ROWS_POINTNORMAL ? 7 : 3; }
static inline int64_t row_bound(int32_t kind) {
  switch (kind) {
    case PCP_ROWS_XYZI: return 4 * ascii::kMaxFloat + 4;                                      // 60
    case PCP_ROWS_XYZRGB: return 3 * ascii::kMaxFloat + ascii::kMaxU32 + 4;                    // 56
    case PCP_ROWS_XYZRGBMASK: return 3 * ascii::kMaxFloat + ascii::kMaxU32 + 5 + 5;            // 62 (mask <= 65535)
    case PCP_ROWS_POINTNORMAL: return 7 * ascii::kMaxFloat + 7;                               // 105
    default: return -1;
  }
}

// Where the columns of text row i are: float column c at col[c][s * stride[c]], s = index ? index[i] : i (the compaction's
// index list over the uploaded planes; nullptr for rows that are stored in order).  The colour is either three bytes
// r g b per row or the packed result word r | g<<8 | b<<16 | has<<24; the mask either uint16 per row or the low byte of
// the fused label word.
struct AsciiSrc {
  const float *col[7];
  int64_t stride[7];
  const int32_t *index;
  const uint8_t *rgb3;
  const uint32_t *packed;
  const uint16_t *mask16;
  const uint32_t *label32;
};

template <int KIND>
struct RowOf {
  static constexpr int kFloats = KIND == PCP_ROWS_XYZI ? 4 : KIND == PCP_ROWS_POINTNORMAL ? 7 : 3;
  static constexpr bool kRgb = KIND == PCP_ROWS_XYZRGB || KIND == PCP_ROWS_XYZRGBMASK;
  static constexpr bool kMask = KIND == PCP_ROWS_XYZRGBMASK;
};

template <int KIND>
struct RowData {
  float f[RowOf<KIND>::kFloats];
  uint32_t rgb, mask;
};

template <int KIND>
__host__ __device__ __forceinline__ RowData<KIND> load_row(const AsciiSrc &s, int64_t i) {
  RowData<KIND> r;
  const int64_t src = s.index ? static_cast<int64_t>(s.index[i]) : i;
#pragma unroll
  for (int c = 0; c < RowOf<KIND>::kFloats; ++c) r.f[c] = s.col[c][src * s.stride[c]];
  r.rgb = 0;
  r.mask = 0;
  if (RowOf<KIND>::kRgb) {
    if (s.packed) {
      const uint32_t v = s.packed[src];
      r.rgb = ascii::rgb_word(v & 0xffu, (v >> 8) & 0xffu, (v >> 16) & 0xffu);
    } else {
      r.rgb = ascii::rgb_word(s.rgb3[3 * src], s.rgb3[3 * src + 1], s.rgb3[3 * src + 2]);
    }
  }
  if (RowOf<KIND>::kMask) r.mask = s.label32 ? (s.label32[src] & 0xffu) : static_cast<uint32_t>(s.mask16[src]);
  return r;
}

template <int KIND>
__host__ __device__ __forceinline__ int row_length(const RowData<KIND> &r) {
  int n = RowOf<KIND>::kFloats;  // the separators and the newline
#pragma unroll
  for (int c = 0; c < RowOf<KIND>::kFloats; ++c) n += ascii::len_g8(r.f[c]);
  if (RowOf<KIND>::kRgb) n += 1 + ascii::len_u32(r.rgb);
  if (RowOf<KIND>::kMask) n += 1 + ascii::len_u32(r.mask);
  return n;
}

template <int KIND, class Ptr>
__host__ __device__ __forceinline__ int row_emit(const RowData<KIND> &r, Ptr dst) {
  int n = 0;
#pragma unroll
  for (int c = 0; c < RowOf<KIND>::kFloats; ++c) {
    if (c) dst[n++] = ' ';
    n += ascii::put_g8(r.f[c], dst + n);
  }
  if (RowOf<KIND>::kRgb) {
    dst[n++] = ' ';
    n += ascii::put_u32(r.rgb, dst + n);
  }
  if (RowOf<KIND>::kMask) {
    dst[n++] = ' ';
    n += ascii::put_u32(r.mask, dst + n);
  }
  dst[n++] = '\n';
  return n;
}

// exclusive prefix of v over the workgroup's lanes (kAsBlock), *total = the sum; ws: kAsBlock / 64 words of LDS
__device__ __forceinline__ uint32_t as_block_exclusive(uint32_t v, uint32_t *total, uint32_t *ws) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) ws[wid] = incl;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kAsBlock / 64; ++k) {
    if (k < wid) base += ws[k];
    tot += ws[k];
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

template <int KIND>
__global__ __launch_bounds__(kAsBlock) void k_ascii_len(AsciiSrc s, int64_t n, uint8_t *__restrict__ len,
                                                        unsigned long long *__restrict__ tile_bytes) {
  __shared__ uint32_t ws[kAsBlock / 64];
  const int64_t tiles = (n + kAsBlock - 1) / kAsBlock;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kAsBlock + threadIdx.x;
    uint32_t l = 0;
    if (i < n) {
      l = static_cast<uint32_t>(row_length<KIND>(load_row<KIND>(s, i)));
      len[i] = static_cast<uint8_t>(l);
    }
    uint32_t total;
    (void)as_block_exclusive(l, &total, ws);
    if (threadIdx.x == 0) tile_bytes[tile] = total;
  }
}

// in place: tile[t] = bytes of the tiles before t, tile[tiles] = all bytes
__global__ __launch_bounds__(kAsScanBlock) void k_ascii_scan(unsigned long long *__restrict__ tile, int64_t tiles) {
  __shared__ unsigned long long ws[kAsScanBlock / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (int64_t base = 0; base < tiles; base += kAsScanBlock) {
    const int64_t i = base + threadIdx.x;
    const unsigned long long v = i < tiles ? tile[i] : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) ws[wid] = incl;
    __syncthreads();
    unsigned long long before = 0, round = 0;
#pragma unroll
    for (int k = 0; k < kAsScanBlock / 64; ++k) {
      if (k < wid) before += ws[k];
      round += ws[k];
    }
    __syncthreads();
    if (i < tiles) tile[i] = carry + before + incl - v;
    carry += round;
  }
  if (threadIdx.x == 0) tile[tiles] = carry;
}

// out[j] = prefix at tile min(j * step, tiles), j < count
__global__ __launch_bounds__(kAsBlock) void k_ascii_pick(const unsigned long long *__restrict__ tile, int64_t tiles, int64_t step,
                                                         unsigned long long *__restrict__ out, int64_t count) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kAsBlock + threadIdx.x;
  if (j < count) out[j] = tile[min(j * step, tiles)];
}

// Tiles [tile_begin, tile_end): the text of tile t goes to text[tile_off[t] - base, ...).  The rows are assembled in LDS at
// the destination's residue mod 16, so that 16-byte words of LDS are 16-byte words of the destination.
template <int KIND>
__global__ __launch_bounds__(kAsBlock) void k_ascii_emit(AsciiSrc s, int64_t n, const uint8_t *__restrict__ len,
                                                         const unsigned long long *__restrict__ tile_off, unsigned long long base,
                                                         int64_t tile_begin, int64_t tile_end, char *__restrict__ text) {
  constexpr int kWords = (kAsBlock * kAsMaxRow + 16 + 15) / 16;
  __shared__ uint4 buf4[kWords];
  __shared__ uint32_t ws[kAsBlock / 64];
  char *buf = reinterpret_cast<char *>(buf4);
  for (int64_t tile = tile_begin + blockIdx.x; tile < tile_end; tile += gridDim.x) {
    const int64_t i = tile * kAsBlock + threadIdx.x;
    const uint32_t l = i < n ? len[i] : 0u;
    uint32_t total;
    const uint32_t off = as_block_exclusive(l, &total, ws);
    char *dst = text + (tile_off[tile] - base);
    const uint32_t shift = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) & 15u);
    if (i < n) (void)row_emit<KIND>(load_row<KIND>(s, i), buf + shift + off);
    __syncthreads();
    // LDS position p is destination byte dst - shift + p; the text is [shift, end)
    const uint32_t end = shift + total;
    const uint32_t v0 = min((shift + 15u) & ~15u, end), v1 = max(end & ~15u, v0);
    char *g = dst - shift;
    for (uint32_t p = shift + threadIdx.x; p < v0; p += kAsBlock) g[p] = buf[p];
    for (uint32_t p = v0 + 16u * threadIdx.x; p < v1; p += 16u * kAsBlock)
      *reinterpret_cast<uint4 *>(g + p) = buf4[p >> 4];
    for (uint32_t p = v1 + threadIdx.x; p < end; p += kAsBlock) g[p] = buf[p];
    __syncthreads();
  }
}

hipError_t preload_ascii() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_ascii_scan));
}

template <int KIND>
static void launch_len(pcp_context *ctx, const AsciiSrc &s, int64_t n, uint32_t grid) {
  hipLaunchKernelGGL(k_ascii_len<KIND>, dim3(grid), dim3(kAsBlock), 0, ctx->stream, s, n, ctx->ascii_len.p, ctx->ascii_tiles.p);
}
template <int KIND>
static void launch_emit(pcp_context *ctx, const AsciiSrc &s, int64_t n, unsigned long long base, int64_t t0, int64_t t1) {
  const uint32_t grid = static_cast<uint32_t>(std::min<int64_t>(t1 - t0, int64_t(1) << 20));
  hipLaunchKernelGGL(k_ascii_emit<KIND>, dim3(grid), dim3(kAsBlock), 0, ctx->stream, s, n, ctx->ascii_len.p, ctx->ascii_tiles.p, base,
                     t0, t1, reinterpret_cast<char *>(ctx->ascii_text.p));
}

// n > 0 rows described by `s` (device memory) as text into out_text (host): lengths, prefix, the byte count, then window by
// window through the context's text buffer.  *bytes = the exact count even when capacity is too small (PCP_ERR_RANGE, nothing
// written).
static int ascii_run(pcp_context *ctx, const char *who, int32_t kind, const AsciiSrc &s, int64_t n, int64_t capacity, char *out_text,
                     int64_t *bytes) {
  const int64_t tiles = div_up(n, kAsBlock);
  const int64_t bound = row_bound(kind);
  const int64_t win_tiles = std::max<int64_t>(1, std::min<int64_t>(tiles, kAsWindowBytes / (bound * kAsBlock)));
  const int64_t windows = div_up(tiles, win_tiles);
  PCP_HIP_TRY(ctx, ctx->ascii_len.ensure(static_cast<size_t>(n) + 16));
  PCP_HIP_TRY(ctx, ctx->ascii_tiles.ensure(static_cast<size_t>(tiles + 1 + windows + 1)));
  unsigned long long *d_pick = ctx->ascii_tiles.p + tiles + 1;
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    const uint32_t grid = static_cast<uint32_t>(std::min<int64_t>(tiles, int64_t(1) << 20));
    switch (kind) {
      case PCP_ROWS_XYZI: launch_len<PCP_ROWS_XYZI>(ctx, s, n, grid); break;
      case PCP_ROWS_XYZRGB: launch_len<PCP_ROWS_XYZRGB>(ctx, s, n, grid); break;
      case PCP_ROWS_XYZRGBMASK: launch_len<PCP_ROWS_XYZRGBMASK>(ctx, s, n, grid); break;
      default: launch_len<PCP_ROWS_POINTNORMAL>(ctx, s, n, grid); break;
    }
    hipLaunchKernelGGL(k_ascii_scan, dim3(1), dim3(kAsScanBlock), 0, ctx->stream, ctx->ascii_tiles.p, tiles);
    hipLaunchKernelGGL(k_ascii_pick, dim3(static_cast<uint32_t>(div_up(windows + 1, kAsBlock))), dim3(kAsBlock), 0, ctx->stream,
                       ctx->ascii_tiles.p, tiles, win_tiles, d_pick, windows + 1);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  std::vector<unsigned long long> edge(static_cast<size_t>(windows) + 1);
  PCP_HIP_TRY(ctx, hipMemcpyAsync(edge.data(), d_pick, edge.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const int64_t total = static_cast<int64_t>(edge.back());
  *bytes = total;
  if (capacity < total)
    return set_error(ctx, PCP_ERR_RANGE, "%s: %lld bytes of text, capacity %lld", who, static_cast<long long>(total),
                     static_cast<long long>(capacity));
  if (!out_text) return set_error(ctx, PCP_ERR_INVALID, "%s: out_text is NULL", who);
  int64_t widest = 0;
  for (int64_t w = 0; w < windows; ++w) widest = std::max<int64_t>(widest, static_cast<int64_t>(edge[static_cast<size_t>(w) + 1] - edge[static_cast<size_t>(w)]));
  PCP_HIP_TRY(ctx, ctx->ascii_text.ensure(static_cast<size_t>(widest) + 16));
  for (int64_t w = 0; w < windows; ++w) {
    const unsigned long long b0 = edge[static_cast<size_t>(w)], b1 = edge[static_cast<size_t>(w) + 1];
    if (b1 == b0) continue;
    const int64_t t0 = w * win_tiles, t1 = std::min(tiles, t0 + win_tiles);
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      switch (kind) {
        case PCP_ROWS_XYZI: launch_emit<PCP_ROWS_XYZI>(ctx, s, n, b0, t0, t1); break;
        case PCP_ROWS_XYZRGB: launch_emit<PCP_ROWS_XYZRGB>(ctx, s, n, b0, t0, t1); break;
        case PCP_ROWS_XYZRGBMASK: launch_emit<PCP_ROWS_XYZRGBMASK>(ctx, s, n, b0, t0, t1); break;
        default: launch_emit<PCP_ROWS_POINTNORMAL>(ctx, s, n, b0, t0, t1); break;
      }
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_text + b0, ctx->ascii_text.p, static_cast<size_t>(b1 - b0), hipMemcpyDeviceToHost, ctx->stream));
  }
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

// the argument rules the row calls share; *out_bytes = 0 on the way in
static int ascii_args(pcp_context *ctx, const char *who, int64_t capacity, int64_t *out_bytes) {
  if (out_bytes) *out_bytes = 0;
  if (capacity < 0) return set_error(ctx, PCP_ERR_INVALID, "%s: negative capacity", who);
  return PCP_OK;
}

// the window [first_row, first_row + max_rows) of m rows
static inline int64_t window_rows(int64_t m, int64_t first_row, int64_t max_rows) {
  return first_row >= m ? 0 : std::min(max_rows, m - first_row);
}

template <int KIND>
static int64_t host_rows(const AsciiSrc &s, int64_t n, char *out) {
  int64_t bytes = 0;
  for (int64_t i = 0; i < n; ++i) {
    const RowData<KIND> r = load_row<KIND>(s, i);
    bytes += out ? row_emit<KIND>(r, out + bytes) : row_length<KIND>(r);
  }
  return bytes;
}
static int64_t host_rows_of(int32_t kind, const AsciiSrc &s, int64_t n, char *out) {
  switch (kind) {
    case PCP_ROWS_XYZI: return host_rows<PCP_ROWS_XYZI>(s, n, out);
    case PCP_ROWS_XYZRGB: return host_rows<PCP_ROWS_XYZRGB>(s, n, out);
    case PCP_ROWS_XYZRGBMASK: return host_rows<PCP_ROWS_XYZRGBMASK>(s, n, out);
    default: return host_rows<PCP_ROWS_POINTNORMAL>(s, n, out);
  }
}

// rows stored in order, row-major floats
static AsciiSrc rows_in_order(int32_t kind, const float *f, const uint8_t *rgb, const uint16_t *mask) {
  AsciiSrc s{};
  const int nf = row_floats(kind);
  for (int c = 0; c < nf; ++c) {
    s.col[c] = f + c;
    s.stride[c] = nf;
  }
  s.rgb3 = rgb;
  s.mask16 = mask;
  return s;
}

// kind known, the arrays the kind reads present
static const char *rows_args_problem(int32_t kind, int64_t n, const float *f, const uint8_t *rgb, const uint16_t *mask) {
  if (row_bound(kind) < 0) return "unknown kind";
  if (n < 0) return "negative row count";
  if (n == 0) return nullptr;
  if (!f) return "f is NULL";
  if ((kind == PCP_ROWS_XYZRGB || kind == PCP_ROWS_XYZRGBMASK) && !rgb) return "rgb is NULL";
  if (kind == PCP_ROWS_XYZRGBMASK && !mask) return "mask is NULL";
  return nullptr;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int64_t pcp_ascii_row_bound(int32_t kind) { return row_bound(kind); }

int pcp_ascii_rows_host(int32_t kind, int64_t n, const float *f, const uint8_t *rgb, const uint16_t *mask, int64_t capacity,
                        char *out_text, int64_t *out_bytes) {
  if (out_bytes) *out_bytes = 0;
  if (const char *why = rows_args_problem(kind, n, f, rgb, mask)) {
    set_global_error("pcp_ascii_rows_host: %s", why);
    return PCP_ERR_INVALID;
  }
  if (capacity < 0) {
    set_global_error("pcp_ascii_rows_host: negative capacity");
    return PCP_ERR_INVALID;
  }
  if (n == 0) return PCP_OK;
  const AsciiSrc s = rows_in_order(kind, f, rgb, mask);
  const int64_t bytes = host_rows_of(kind, s, n, nullptr);
  if (out_bytes) *out_bytes = bytes;
  if (capacity < bytes) {
    set_global_error("pcp_ascii_rows_host: %lld bytes of text, capacity %lld", static_cast<long long>(bytes),
                     static_cast<long long>(capacity));
    return PCP_ERR_RANGE;
  }
  if (!out_text) {
    set_global_error("pcp_ascii_rows_host: out_text is NULL");
    return PCP_ERR_INVALID;
  }
  (void)host_rows_of(kind, s, n, out_text);
  return PCP_OK;
}

int pcp_ascii_rows(pcp_context *ctx, int32_t kind, int64_t n, const float *f, const uint8_t *rgb, const uint16_t *mask,
                   int64_t capacity, char *out_text, int64_t *out_bytes) {
  if (!ctx) return PCP_ERR_INVALID;
  int rc = ascii_args(ctx, "pcp_ascii_rows", capacity, out_bytes);
  if (rc != PCP_OK) return rc;
  if (const char *why = rows_args_problem(kind, n, f, rgb, mask)) return set_error(ctx, PCP_ERR_INVALID, "pcp_ascii_rows: %s", why);
  if (n == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // floats | rgb | mask, each section from a 16-byte boundary
  const size_t sn = static_cast<size_t>(n), fbytes = sn * static_cast<size_t>(row_floats(kind)) * 4;
  const bool has_rgb = kind == PCP_ROWS_XYZRGB || kind == PCP_ROWS_XYZRGBMASK, has_mask = kind == PCP_ROWS_XYZRGBMASK;
  const size_t rgb_off = (fbytes + 15) & ~size_t(15), mask_off = (rgb_off + (has_rgb ? 3 * sn : 0) + 15) & ~size_t(15);
  PCP_HIP_TRY(ctx, ctx->ascii_in.ensure(mask_off + (has_mask ? 2 * sn : 0) + 16));
  uint8_t *d = ctx->ascii_in.p;
  PCP_HIP_TRY(ctx, hipMemcpyAsync(d, f, fbytes, hipMemcpyHostToDevice, ctx->stream));
  if (has_rgb) PCP_HIP_TRY(ctx, hipMemcpyAsync(d + rgb_off, rgb, 3 * sn, hipMemcpyHostToDevice, ctx->stream));
  if (has_mask) PCP_HIP_TRY(ctx, hipMemcpyAsync(d + mask_off, mask, 2 * sn, hipMemcpyHostToDevice, ctx->stream));
  const AsciiSrc s = rows_in_order(kind, reinterpret_cast<const float *>(d), has_rgb ? d + rgb_off : nullptr,
                                   has_mask ? reinterpret_cast<const uint16_t *>(d + mask_off) : nullptr);
  int64_t bytes = 0;
  rc = ascii_run(ctx, "pcp_ascii_rows", kind, s, n, capacity, out_text, &bytes);
  if (out_bytes) *out_bytes = bytes;
  return rc;
}

int pcp_colour_compact_ascii(pcp_context *ctx, int32_t with_label, int64_t first_row, int64_t max_rows, int64_t capacity,
                             char *out_text, int64_t *out_rows, int64_t *out_bytes) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  int rc = ascii_args(ctx, "pcp_colour_compact_ascii", capacity, out_bytes);
  if (rc != PCP_OK) return rc;
  if (first_row < 0 || max_rows < 0) return set_error(ctx, PCP_ERR_INVALID, "pcp_colour_compact_ascii: negative row window");
  if (!ctx->colour_result_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_colour_compact_ascii: no result (call pcp_colorize / pcp_colorize_from_depth / pcp_colour_finalise)");
  if (with_label && !ctx->labels_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_colour_compact_ascii: with_label asked of a result made without label fusion (pcp_set_label_fusion)");
  const int64_t n = ctx->n;
  if (n == 0 || max_rows == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int64_t m = 0;
  rc = colour_compact_indices(ctx, &m);  // the list pcp_colour_compact gathers by, in ctx->s_cell
  if (rc != PCP_OK) return rc;
  const int64_t rows = window_rows(m, first_row, max_rows);
  if (rows == 0) return PCP_OK;
  const size_t plane = (static_cast<size_t>(n) + 3) & ~size_t(3);
  AsciiSrc s{};
  for (int c = 0; c < 3; ++c) {
    s.col[c] = ctx->xyz.p + static_cast<size_t>(c) * plane;
    s.stride[c] = 1;
  }
  s.index = ctx->s_cell.p + first_row;
  s.packed = ctx->rgba2[ctx->rgba_cur].p;
  s.label32 = with_label ? ctx->labels.p : nullptr;
  int64_t bytes = 0;
  rc = ascii_run(ctx, "pcp_colour_compact_ascii", with_label ? PCP_ROWS_XYZRGBMASK : PCP_ROWS_XYZRGB, s, rows, capacity, out_text, &bytes);
  if (out_bytes) *out_bytes = bytes;
  if (rc == PCP_OK && out_rows) *out_rows = rows;
  return rc;
}

int pcp_mls_fetch_ascii(pcp_context *ctx, int64_t first_row, int64_t max_rows, int64_t capacity, char *out_text, int64_t *out_rows,
                        int64_t *out_bytes) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  int rc = ascii_args(ctx, "pcp_mls_fetch_ascii", capacity, out_bytes);
  if (rc != PCP_OK) return rc;
  if (first_row < 0 || max_rows < 0) return set_error(ctx, PCP_ERR_INVALID, "pcp_mls_fetch_ascii: negative row window");
  const int64_t rows = window_rows(ctx->mls_count, first_row, max_rows);
  if (rows == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  AsciiSrc s{};
  for (int c = 0; c < 3; ++c) {
    s.col[c] = ctx->mls_xyz.p + 3 * first_row + c;
    s.stride[c] = 3;
    s.col[3 + c] = ctx->mls_normal.p + 3 * first_row + c;
    s.stride[3 + c] = 3;
  }
  s.col[6] = ctx->mls_curv.p + first_row;
  s.stride[6] = 1;
  int64_t bytes = 0;
  rc = ascii_run(ctx, "pcp_mls_fetch_ascii", PCP_ROWS_POINTNORMAL, s, rows, capacity, out_text, &bytes);
  if (out_bytes) *out_bytes = bytes;
  if (rc == PCP_OK && out_rows) *out_rows = rows;
  return rc;
}

}  // extern "C"
