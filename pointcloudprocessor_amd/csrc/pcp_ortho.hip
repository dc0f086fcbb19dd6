// pcp_ortho.hip -- orthographic maps of the coloured cloud ("Orthographic maps", OM1-OM8): one metric picture of
// the surface at a fixed number of metres per pixel -- colour, depth, point index, fused label -- accumulated on the device
// over any number of colour results (one-shot runs, the chunks of the streamed chain).  Per pixel the nearest contributor
// wins through one 64-bit atomicMin on (ord(depth) << 32 | global index), the reduction of k_gm_scatter; a second pass with
// plain stores writes the winners' payload; the optional fill takes empty pixels from their nearest occupied one through the
// exact distance transform of pcp_mask_edt.hip.  The arithmetic is pcp_ortho.hpp's, shared with pcp_ortho_host.  A second
// kind of frame, a cylinder unrolled along its arc ("Cylindrical facets", CY1-CY9; pcp_ortho_cyl.hpp), differs in
// the pixel alone: pcp_ortho_begin_cyl, pcp_ortho_cyl_host and the closed-form fit pcp_cyl_fit_host.
// Opt-in: nothing here runs unless one of its entry points is called.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <new>
#include <type_traits>
#include <vector>

#include "pcp_eigen33_host.hpp"
#include "pcp_internal.hpp"
#include "pcp_mask_edt.hpp"
#include "pcp_ortho.hpp"
#include "pcp_ortho_cyl.hpp"

namespace pcp {

constexpr int kOrBlock = 256;
constexpr int64_t kOrMaxGrid = 4096;  // workgroups of the grid-stride passes
// device scalars of the accumulator
enum { OR_CONTRIBUTORS = 0, OR_ATOMICS, OR_OCCUPIED, OR_FILLED, OR_SCALARS };

// the contributor of lane j of the upload's spatial order (sxyz / perm: the uploaded coordinates; the packed word of the
// input-order result): its pixel (-1: none), key, input row and word.  kFacet (pcp_ortho_add_facet): only the rows whose
// facet label (input order) is facet_id contribute.  kCyl (pcp_ortho_begin_cyl): the frame is a cylinder's and the pixel
// comes from pcp_ortho_cyl.hpp (CY2); everything after the pixel is the same.
template <bool kCyl>
using OrFrame = std::conditional_t<kCyl, cy::Frame, om::Frame>;

template <bool kFacet, bool kCyl>
__device__ __forceinline__ int32_t or_contributor(int64_t j, int64_t n, const float *__restrict__ sx, const float *__restrict__ sy,
                                                  const float *__restrict__ sz, const int32_t *__restrict__ perm,
                                                  const uint32_t *__restrict__ packed, [[maybe_unused]] const int32_t *__restrict__ facet,
                                                  [[maybe_unused]] int32_t facet_id, const OrFrame<kCyl> &f, uint32_t index_base,
                                                  unsigned long long *key, int32_t *row, uint32_t *word) {
  *key = om::kEmptyKey;
  if (j >= n) return -1;
  const int32_t i = perm[j];
  if constexpr (kFacet) {
    if (facet[i] != facet_id) return -1;
  }
  const uint32_t w = packed[i];
  if (!(w >> 24)) return -1;
  int32_t pixel;
  uint32_t depth_bits;
  if constexpr (kCyl) {
    if (!cy::project(f, sx[j], sy[j], sz[j], &pixel, &depth_bits)) return -1;
  } else {
    if (!om::project(f, sx[j], sy[j], sz[j], &pixel, &depth_bits)) return -1;
  }
  *row = i;
  *word = w;
  *key = om::key_of(depth_bits, index_base + static_cast<uint32_t>(i));
  return pixel;
}

// OM3.  One lane per row.  Equal pixels of neighbouring lanes are merged before the atomic: a lane without a contributor joins
// the run of the nearest lane below that has one (and brings the empty key, the minimum's identity); the smallest key of a run
// of equal pixels is found by a segmented suffix minimum (six shuffle steps) and the run's first lane issues the one atomic.
// (One atomic per contributor instead: the same add 0.71 -> 1.99 ms where 200 points share a pixel, profiles/ortho_probe.md.)
template <bool kFacet, bool kCyl>
__global__ __launch_bounds__(kOrBlock) void k_or_scatter(int64_t n, const float *__restrict__ sx, const float *__restrict__ sy,
                                                         const float *__restrict__ sz, const int32_t *__restrict__ perm,
                                                         const uint32_t *__restrict__ packed, const int32_t *__restrict__ facet,
                                                         int32_t facet_id, OrFrame<kCyl> f, uint32_t index_base,
                                                         unsigned long long *__restrict__ keys, unsigned long long *__restrict__ scalars) {
  const int lane = static_cast<int>(threadIdx.x & 63u);
  uint32_t contributors = 0u, atomics = 0u;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kOrBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kOrBlock) {
    unsigned long long key;
    int32_t row = 0;
    uint32_t word = 0u;
    const int32_t pixel = or_contributor<kFacet, kCyl>(base + threadIdx.x, n, sx, sy, sz, perm, packed, facet, facet_id, f, index_base, &key, &row, &word);
    contributors += pixel >= 0 ? 1u : 0u;
    const unsigned long long with = __ballot(pixel >= 0);
    if (!with) continue;  // (the same in every lane of the wavefront)
    const unsigned long long below = with & ((1ull << lane) - 1ull);
    const int src = (pixel < 0 && below) ? 63 - __clzll(static_cast<long long>(below)) : lane;
    const int32_t run_pixel = __shfl(pixel, src, 64);
    const int32_t before = __shfl_up(run_pixel, 1, 64);
    const bool head = lane == 0 || before != run_pixel;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int run_end = above ? lane + (__ffsll(above) - 1) : 63;  // last lane of this lane's run
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long other = __shfl_down(key, d, 64);
      if (lane + d <= run_end) key = other < key ? other : key;
    }
    if (head && run_pixel >= 0) {  // (such a head is a lane with a contributor of its own: pixel == run_pixel)
      atomicMin(keys + run_pixel, key);
      atomics += 1u;
    }
  }
  const unsigned long long both = wave_sum_u64((static_cast<unsigned long long>(atomics) << 32) | contributors);  // (n < 2^31 rows)
  if (lane == 0 && both) {
    atomicAdd(scalars + OR_CONTRIBUTORS, both & 0xffffffffull);
    atomicAdd(scalars + OR_ATOMICS, both >> 32);
  }
}

// OM4.  The same contributors, after the scatter: the one whose key is its pixel's key stores the payload word.  No atomics.
template <bool kLabel, bool kFacet, bool kCyl>
__global__ __launch_bounds__(kOrBlock) void k_or_payload(int64_t n, const float *__restrict__ sx, const float *__restrict__ sy,
                                                         const float *__restrict__ sz, const int32_t *__restrict__ perm,
                                                         const uint32_t *__restrict__ packed,
                                                         [[maybe_unused]] const uint32_t *__restrict__ labels,
                                                         const int32_t *__restrict__ facet, int32_t facet_id, OrFrame<kCyl> f,
                                                         uint32_t index_base, const unsigned long long *__restrict__ keys,
                                                         uint32_t *__restrict__ payload) {
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kOrBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kOrBlock) {
    unsigned long long key;
    int32_t row = 0;
    uint32_t word = 0u;
    const int32_t pixel = or_contributor<kFacet, kCyl>(base + threadIdx.x, n, sx, sy, sz, perm, packed, facet, facet_id, f, index_base, &key, &row, &word);
    if (pixel < 0 || keys[pixel] != key) continue;
    uint32_t label = 0u;
    if constexpr (kLabel) label = labels[row] & 0xffu;
    payload[pixel] = om::payload_of(word, label);
  }
}

// OM6.  The bit image k_md_columns reads, from the key image: one lane per (column, segment of 64 rows); bit j of the word =
// pixel (x, 64 * s + j) is occupied (the distance transform's background); rows past the map stay 0.
__global__ __launch_bounds__(kOrBlock) void k_or_bits(const unsigned long long *__restrict__ keys, int32_t w, int32_t h, int32_t segs,
                                                      unsigned long long *__restrict__ bits) {
  const int32_t x = static_cast<int32_t>(blockIdx.x) * kOrBlock + static_cast<int32_t>(threadIdx.x);
  if (x >= w) return;
  const int32_t s = static_cast<int32_t>(blockIdx.y);
  if (s >= segs) return;
  const int32_t y0 = s * md::kSegmentRows, y1 = min(h, y0 + md::kSegmentRows);
  unsigned long long m = 0;
  for (int32_t y = y0; y < y1; ++y)
    if (keys[static_cast<int64_t>(y) * w + x] != om::kEmptyKey) m |= 1ull << (y - y0);
  bits[static_cast<int64_t>(s) * w + x] = m;
}

// OM6.  The pixel every pixel takes its values from: itself when occupied, its nearest occupied pixel when that lies within
// the radius (d2 / nearest: the distance transform; nullptr with radius 0), else -1.  Counts both kinds.
__global__ __launch_bounds__(kOrBlock) void k_or_source(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ d2,
                                                        const int32_t *__restrict__ nearest, int64_t pixels, int32_t radius,
                                                        int32_t *__restrict__ source, unsigned long long *__restrict__ scalars) {
  uint32_t occupied = 0u, filled = 0u;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kOrBlock + threadIdx.x; p < pixels; p += static_cast<int64_t>(gridDim.x) * kOrBlock) {
    int32_t src;
    if (keys[p] != om::kEmptyKey) {
      src = static_cast<int32_t>(p);
      occupied += 1u;
    } else {
      src = d2 ? om::fill_source(d2[p], nearest[p], radius) : -1;
      filled += src >= 0 ? 1u : 0u;
    }
    source[p] = src;
  }
  const unsigned long long both = wave_sum_u64((static_cast<unsigned long long>(filled) << 32) | occupied);  // (< 2^32 pixels each)
  if ((threadIdx.x & 63u) == 0u && both) {
    atomicAdd(scalars + OR_OCCUPIED, both & 0xffffffffull);
    atomicAdd(scalars + OR_FILLED, both >> 32);
  }
}

// OM7.  The layers a fetch asked for (nullptr: not asked), gathered through the source image.
__global__ __launch_bounds__(kOrBlock) void k_or_layers(int64_t pixels, const int32_t *__restrict__ source,
                                                        const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ payload,
                                                        uint32_t *__restrict__ out_index, float *__restrict__ out_depth,
                                                        uint8_t *__restrict__ out_rgb, uint8_t *__restrict__ out_label,
                                                        uint8_t *__restrict__ out_status) {
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kOrBlock + threadIdx.x; p < pixels; p += static_cast<int64_t>(gridDim.x) * kOrBlock) {
    const int32_t src = source[p];
    uint32_t index = om::kNoIndex, word = 0u;
    float depth = 0.0f;
    if (src >= 0) {
      const unsigned long long key = keys[src];
      index = om::key_index(key);
      depth = om::key_depth(key);
      word = payload[src];
    }
    if (out_index) out_index[p] = index;
    if (out_depth) out_depth[p] = depth;
    if (out_rgb) {
      out_rgb[3 * p] = static_cast<uint8_t>(word);
      out_rgb[3 * p + 1] = static_cast<uint8_t>(word >> 8);
      out_rgb[3 * p + 2] = static_cast<uint8_t>(word >> 16);
    }
    if (out_label) out_label[p] = static_cast<uint8_t>(word >> 24);
    if (out_status) out_status[p] = src < 0 ? 0 : (src == p ? 1 : 2);
  }
}

hipError_t preload_ortho() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_or_source));
}

static inline uint32_t or_blocks(int64_t n) {
  return static_cast<uint32_t>(std::max<int64_t>(1, std::min<int64_t>(div_up(n, kOrBlock), kOrMaxGrid)));
}

static om::Frame or_frame(const pcp_ortho_frame &c) {
  om::Frame f;
  for (int a = 0; a < 3; ++a) {
    f.o[a] = c.o[a];
    f.u[a] = c.u[a];
    f.v[a] = c.v[a];
    f.n[a] = c.n[a];
  }
  f.inv = om::inverse_gsd(c.gsd);
  f.w = c.width;
  f.h = c.height;
  f.wf = static_cast<float>(c.width);
  f.hf = static_cast<float>(c.height);
  f.d_min = c.d_min;
  f.d_max = c.d_max;
  return f;
}

static cy::Frame or_cyl_frame(const pcp_cyl_frame &c) { return cy::make_frame(c); }

// OM1 for either form; msg receives the refusal
static int or_check_frame(const char *who, const pcp_ortho_frame *fr, char *msg, size_t cap) {
  const char *why = "";
  double fit = 0.0;
  const int bad = om::frame_check(fr->o, fr->u, fr->v, fr->n, fr->gsd, fr->width, fr->height, fr->d_min, fr->d_max, &why, &fit);
  if (bad == 1) {
    std::snprintf(msg, cap, "%s: %s", who, why);
    return PCP_ERR_INVALID;
  }
  if (bad == 2) {
    std::snprintf(msg, cap, "%s: raster %d x %d at gsd %g: %s; the same extent fits at gsd %.6g", who, fr->width, fr->height,
                  static_cast<double>(fr->gsd), why, fit);
    return PCP_ERR_RANGE;
  }
  return PCP_OK;
}

// CY1, the same way
static int or_check_cyl_frame(const char *who, const pcp_cyl_frame *fr, char *msg, size_t cap) {
  const char *why = "";
  double fit = 0.0;
  const int bad = cy::frame_check(fr->c, fr->a, fr->e, fr->b, fr->radius, fr->gsd, fr->width, fr->height, fr->d_min, fr->d_max, fr->side,
                                  &why, &fit);
  if (bad == 1) {
    std::snprintf(msg, cap, "%s: %s", who, why);
    return PCP_ERR_INVALID;
  }
  if (bad == 2) {
    std::snprintf(msg, cap, "%s: raster %d x %d at gsd %g: %s; the same extent fits at gsd %.6g", who, fr->width, fr->height,
                  static_cast<double>(fr->gsd), why, fit);
    return PCP_ERR_RANGE;
  }
  return PCP_OK;
}

static void or_drop(pcp_context *ctx) {
  OrthoMap &m = ctx->ortho;
  ctx->ortho_defects.release();  // SD8: the defects belong to the live map
  m.keys.release();
  m.payload.release();
  m.source.release();
  m.scalars.release();
  m.live = m.finished = m.labels_fixed = m.with_label = m.cyl = false;
  m.contributors = m.atomics = m.occupied = m.filled = m.adds = 0;
  m.fill_radius = 0;
}

// what either begin does once its frame is accepted: drops the live map and starts an empty one of w x h pixels
static int or_start(pcp_context *ctx, int32_t w, int32_t h) {
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  or_drop(ctx);
  OrthoMap &m = ctx->ortho;
  const size_t px = static_cast<size_t>(w) * static_cast<size_t>(h);
  PCP_HIP_TRY(ctx, m.keys.ensure(px + 2));
  PCP_HIP_TRY(ctx, m.payload.ensure(px + 4));
  PCP_HIP_TRY(ctx, m.scalars.ensure(OR_SCALARS));
  PCP_HIP_TRY(ctx, hipMemsetAsync(m.keys.p, 0xff, px * 8, ctx->stream));  // the empty key is all ones
  PCP_HIP_TRY(ctx, hipMemsetAsync(m.payload.p, 0, px * 4, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(m.scalars.p, 0, OR_SCALARS * 8, ctx->stream));
  return PCP_OK;
}

// the two passes of an add over the uploaded cloud with the words `packed` (device, input order) and `labels` (nullable);
// facet (nullable; device, input order): only the rows labelled facet_id
template <bool kFacet, bool kCyl>
static int or_add_passes(pcp_context *ctx, const OrFrame<kCyl> &f, const uint32_t *packed, const uint32_t *labels, const int32_t *facet,
                         int32_t facet_id, uint32_t index_base, int64_t *out_contributors) {
  OrthoMap &m = ctx->ortho;
  const int64_t n = ctx->n;
  const size_t plane = (static_cast<size_t>(n) + 3) & ~size_t(3);
  const float *sx = ctx->sxyz.p, *sy = sx + plane, *sz = sy + plane;
  PCP_HIP_TRY(ctx, hipMemsetAsync(m.scalars.p, 0, 2 * 8, ctx->stream));  // contributors, atomics
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL((k_or_scatter<kFacet, kCyl>), dim3(or_blocks(n)), dim3(kOrBlock), 0, ctx->stream, n, sx, sy, sz, ctx->perm.p, packed, facet,
                       facet_id, f, index_base, m.keys.p, m.scalars.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    if (labels)
      hipLaunchKernelGGL((k_or_payload<true, kFacet, kCyl>), dim3(or_blocks(n)), dim3(kOrBlock), 0, ctx->stream, n, sx, sy, sz, ctx->perm.p, packed,
                         labels, facet, facet_id, f, index_base, m.keys.p, m.payload.p);
    else
      hipLaunchKernelGGL((k_or_payload<false, kFacet, kCyl>), dim3(or_blocks(n)), dim3(kOrBlock), 0, ctx->stream, n, sx, sy, sz, ctx->perm.p, packed,
                         static_cast<const uint32_t *>(nullptr), facet, facet_id, f, index_base, m.keys.p, m.payload.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  unsigned long long h[2];
  PCP_HIP_TRY(ctx, hipMemcpyAsync(h, m.scalars.p, 2 * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  m.contributors += static_cast<int64_t>(h[OR_CONTRIBUTORS]);
  m.atomics += static_cast<int64_t>(h[OR_ATOMICS]);
  if (out_contributors) *out_contributors = static_cast<int64_t>(h[OR_CONTRIBUTORS]);
  return PCP_OK;
}

template <bool kFacet>
static int or_add_words(pcp_context *ctx, const uint32_t *packed, const uint32_t *labels, const int32_t *facet, int32_t facet_id,
                        uint32_t index_base, int64_t *out_contributors) {
  const OrthoMap &m = ctx->ortho;
  if (m.cyl) return or_add_passes<kFacet, true>(ctx, or_cyl_frame(m.cyl_frame), packed, labels, facet, facet_id, index_base, out_contributors);
  return or_add_passes<kFacet, false>(ctx, or_frame(m.frame), packed, labels, facet, facet_id, index_base, out_contributors);
}

// what both adds check before they touch the device
static int or_add_check(pcp_context *ctx, const char *who, int64_t index_base, bool with_label) {
  const OrthoMap &m = ctx->ortho;
  if (!m.live) return set_error(ctx, PCP_ERR_STATE, "%s: no accumulation (call pcp_ortho_begin)", who);
  if (m.finished) return set_error(ctx, PCP_ERR_STATE, "%s: the accumulation is finished (pcp_ortho_begin starts the next)", who);
  if (index_base < 0 || index_base > om::kMaxIndexEnd - ctx->n)  // (index_base + n > 2^32 - 1, without the sum: it may overflow)
    return set_error(ctx, PCP_ERR_RANGE, "%s: index_base %lld with %lld rows: global indices outside 0 .. 2^32 - 2", who,
                     static_cast<long long>(index_base), static_cast<long long>(ctx->n));
  if (m.labels_fixed && with_label != m.with_label)
    return set_error(ctx, PCP_ERR_STATE, "%s: this add comes %s fused labels, the accumulation's first came %s them", who,
                     with_label ? "with" : "without", m.with_label ? "with" : "without");
  return PCP_OK;
}

// ---- pcp_ortho_fit_frame_host: the eigenpairs of a symmetric 3 x 3 matrix by pcp_eigen33_host.hpp's closed form ----
static void or_roots3(const double a[6], double r[3]) { eig::roots3(a, r); }
static void or_eigenvector(const double a[6], double r, double v[3]) { eig::eigenvector(a, r, v); }
static int or_largest_component(const double v[3]) { return eig::largest_component(v); }

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_ortho_begin(pcp_context *ctx, const pcp_ortho_frame *frame) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!frame) return set_error(ctx, PCP_ERR_INVALID, "pcp_ortho_begin: NULL frame");
  char msg[320];
  const int rc = or_check_frame("pcp_ortho_begin", frame, msg, sizeof msg);
  if (rc != PCP_OK) return set_error(ctx, rc, "%s", msg);
  const int brc = or_start(ctx, frame->width, frame->height);
  if (brc != PCP_OK) return brc;
  OrthoMap &m = ctx->ortho;
  m.frame = *frame;
  m.live = true;
  return PCP_OK;
}

int pcp_ortho_begin_cyl(pcp_context *ctx, const pcp_cyl_frame *frame) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!frame) return set_error(ctx, PCP_ERR_INVALID, "pcp_ortho_begin_cyl: NULL frame");
  char msg[320];
  const int rc = or_check_cyl_frame("pcp_ortho_begin_cyl", frame, msg, sizeof msg);
  if (rc != PCP_OK) return set_error(ctx, rc, "%s", msg);
  const int brc = or_start(ctx, frame->width, frame->height);
  if (brc != PCP_OK) return brc;
  OrthoMap &m = ctx->ortho;
  m.frame = pcp_ortho_frame{};  // (finish, fetch and stats read the raster from here)
  m.frame.gsd = frame->gsd;
  m.frame.width = frame->width;
  m.frame.height = frame->height;
  m.cyl_frame = *frame;
  m.cyl = true;
  m.live = true;
  return PCP_OK;
}

int pcp_ortho_add(pcp_context *ctx, int64_t index_base, int64_t *out_contributors) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_contributors) *out_contributors = 0;
  OrthoMap &m = ctx->ortho;
  const bool with_label = ctx->labels_live;
  if (m.live && !m.finished && !ctx->colour_result_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_add: no colour result (call pcp_colorize / pcp_colorize_from_depth / pcp_colour_finalise)");
  int rc = or_add_check(ctx, "pcp_ortho_add", index_base, with_label);
  if (rc != PCP_OK) return rc;
  if (ctx->n > 0) {
    PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = or_add_words<false>(ctx, ctx->rgba2[ctx->rgba_cur].p, with_label ? ctx->labels.p : nullptr, nullptr, 0, static_cast<uint32_t>(index_base),
                             out_contributors);
    if (rc != PCP_OK) return rc;
  }
  m.labels_fixed = true;
  m.with_label = with_label;
  m.adds += 1;
  return PCP_OK;
}

int pcp_ortho_add_facet(pcp_context *ctx, int32_t facet_id, int64_t index_base, int64_t *out_contributors) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_contributors) *out_contributors = 0;
  OrthoMap &m = ctx->ortho;
  const bool with_label = ctx->labels_live;
  if (m.live && !m.finished && !ctx->colour_result_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_add_facet: no colour result (call pcp_colorize / pcp_colorize_from_depth / pcp_colour_finalise)");
  int rc = or_add_check(ctx, "pcp_ortho_add_facet", index_base, with_label);
  if (rc != PCP_OK) return rc;
  if (!ctx->facets.live) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_add_facet: no facets (pcp_facets on this cloud and these normals)");
  if (facet_id < 0 || facet_id >= ctx->n)
    return set_error(ctx, PCP_ERR_RANGE, "pcp_ortho_add_facet: facet %d outside 0 .. %lld", facet_id, static_cast<long long>(ctx->n) - 1);
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = or_add_words<true>(ctx, ctx->rgba2[ctx->rgba_cur].p, with_label ? ctx->labels.p : nullptr, ctx->facets.label.p, facet_id,
                          static_cast<uint32_t>(index_base), out_contributors);
  if (rc != PCP_OK) return rc;
  m.labels_fixed = true;
  m.with_label = with_label;
  m.adds += 1;
  return PCP_OK;
}

int pcp_ortho_add_packed(pcp_context *ctx, const uint32_t *rgba, int64_t index_base, int64_t *out_contributors) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_contributors) *out_contributors = 0;
  OrthoMap &m = ctx->ortho;
  int rc = or_add_check(ctx, "pcp_ortho_add_packed", index_base, false);
  if (rc != PCP_OK) return rc;
  if (ctx->n > 0) {
    if (!ctx->sxyz.p) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_add_packed: no cloud uploaded");
    if (!rgba) return set_error(ctx, PCP_ERR_INVALID, "pcp_ortho_add_packed: NULL words");
    PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf<uint32_t> words;  // the caller's words (host or device memory)
    PCP_HIP_TRY(ctx, words.ensure(static_cast<size_t>(ctx->n) + 4));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(words.p, rgba, static_cast<size_t>(ctx->n) * 4, hipMemcpyDefault, ctx->stream));
    rc = or_add_words<false>(ctx, words.p, nullptr, nullptr, 0, static_cast<uint32_t>(index_base), out_contributors);  // (synchronises: words may go)
    if (rc != PCP_OK) return rc;
  }
  m.labels_fixed = true;
  m.with_label = false;
  m.adds += 1;
  return PCP_OK;
}

int pcp_ortho_finish(pcp_context *ctx, int32_t fill_radius_px, int64_t *out_occupied, int64_t *out_filled) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_occupied) *out_occupied = 0;
  if (out_filled) *out_filled = 0;
  OrthoMap &m = ctx->ortho;
  if (!m.live) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_finish: no accumulation (call pcp_ortho_begin)");
  if (fill_radius_px < 0 || fill_radius_px > om::kMaxFill)
    return set_error(ctx, PCP_ERR_INVALID, "pcp_ortho_finish: fill radius %d outside 0..%d pixels", fill_radius_px, om::kMaxFill);
  ctx->ortho_defects.release();  // SD8: every accepted finish drops the defects of the map
  if (!(m.finished && fill_radius_px == m.fill_radius)) {  // (the key image stays as the adds left it: any radius can follow)
    PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int32_t w = m.frame.width, h = m.frame.height;
    const int64_t px = static_cast<int64_t>(w) * h;
    const int32_t segs = (h + md::kSegmentRows - 1) / md::kSegmentRows;
    PCP_HIP_TRY(ctx, m.source.ensure(static_cast<size_t>(px) + 4));
    // the fill's scratch is its own (the mask distance maps keep theirs) and goes when this call returns
    DevBuf<unsigned long long> bits;
    DevBuf<uint32_t> col, d2;
    DevBuf<int32_t> nearest;
    if (fill_radius_px > 0) {
      PCP_HIP_TRY(ctx, bits.ensure(static_cast<size_t>(segs) * w + 4));
      PCP_HIP_TRY(ctx, col.ensure(static_cast<size_t>(px) + 4));
      PCP_HIP_TRY(ctx, d2.ensure(static_cast<size_t>(px) + 4));
      PCP_HIP_TRY(ctx, nearest.ensure(static_cast<size_t>(px) + 4));
      {
        LaunchTimer t(ctx, PCP_K_MISC);
        hipLaunchKernelGGL(k_or_bits, dim3(static_cast<uint32_t>((w + kOrBlock - 1) / kOrBlock), static_cast<uint32_t>(segs)), dim3(kOrBlock), 0,
                           ctx->stream, m.keys.p, w, h, segs, bits.p);
        PCP_HIP_TRY(ctx, hipGetLastError());
      }
      const int rc = mask_edt_of_bits(ctx, bits.p, w, h, segs, col.p, d2.p, nearest.p);
      if (rc != PCP_OK) return rc;
    }
    PCP_HIP_TRY(ctx, hipMemsetAsync(m.scalars.p + OR_OCCUPIED, 0, 2 * 8, ctx->stream));  // occupied, filled
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_or_source, dim3(or_blocks(px)), dim3(kOrBlock), 0, ctx->stream, m.keys.p,
                         fill_radius_px > 0 ? d2.p : static_cast<const uint32_t *>(nullptr),
                         fill_radius_px > 0 ? nearest.p : static_cast<const int32_t *>(nullptr), px, fill_radius_px, m.source.p, m.scalars.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    unsigned long long hs[2];
    PCP_HIP_TRY(ctx, hipMemcpyAsync(hs, m.scalars.p + OR_OCCUPIED, 2 * 8, hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    m.occupied = static_cast<int64_t>(hs[0]);
    m.filled = static_cast<int64_t>(hs[1]);
    m.fill_radius = fill_radius_px;
    m.finished = true;
  }
  if (out_occupied) *out_occupied = m.occupied;
  if (out_filled) *out_filled = m.filled;
  return PCP_OK;
}

int pcp_ortho_fetch(pcp_context *ctx, uint32_t *out_index, float *out_depth, uint8_t *out_rgb, uint8_t *out_label, uint8_t *out_status,
                    int32_t *out_source) {
  if (!ctx) return PCP_ERR_INVALID;
  OrthoMap &m = ctx->ortho;
  if (!m.live) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_fetch: no accumulation (call pcp_ortho_begin)");
  if (!m.finished) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_fetch: pcp_ortho_finish has not run");
  if (out_label && !m.with_label)
    return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_fetch: out_label asked of an accumulation that holds no labels (pcp_set_label_fusion)");
  if (!(out_index || out_depth || out_rgb || out_label || out_status || out_source)) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t px = static_cast<size_t>(m.frame.width) * static_cast<size_t>(m.frame.height);
  DevBuf<uint32_t> d_index;
  DevBuf<float> d_depth;
  DevBuf<uint8_t> d_rgb, d_label, d_status;
  if (out_index) PCP_HIP_TRY(ctx, d_index.ensure(px + 4));
  if (out_depth) PCP_HIP_TRY(ctx, d_depth.ensure(px + 4));
  if (out_rgb) PCP_HIP_TRY(ctx, d_rgb.ensure(3 * px + 16));
  if (out_label) PCP_HIP_TRY(ctx, d_label.ensure(px + 16));
  if (out_status) PCP_HIP_TRY(ctx, d_status.ensure(px + 16));
  if (out_index || out_depth || out_rgb || out_label || out_status) {
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_or_layers, dim3(or_blocks(static_cast<int64_t>(px))), dim3(kOrBlock), 0, ctx->stream, static_cast<int64_t>(px),
                       m.source.p, m.keys.p, m.payload.p, d_index.p, d_depth.p, d_rgb.p, d_label.p, d_status.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  if (out_index) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_index, d_index.p, 4 * px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_depth) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_depth, d_depth.p, 4 * px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_rgb) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rgb, d_rgb.p, 3 * px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_label) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_label, d_label.p, px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_status) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_status, d_status.p, px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_source) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_source, m.source.p, 4 * px, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the layers' device copies are freed on return)
  return PCP_OK;
}

int pcp_ortho_stats(pcp_context *ctx, int64_t out[6]) {
  if (!ctx || !out) return PCP_ERR_INVALID;
  const OrthoMap &m = ctx->ortho;
  if (!m.live) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_stats: no accumulation (call pcp_ortho_begin)");
  out[0] = m.contributors;
  out[1] = m.atomics;
  out[2] = m.occupied;
  out[3] = m.filled;
  out[4] = m.adds;
  out[5] = static_cast<int64_t>(m.frame.width) * m.frame.height;
  return PCP_OK;
}

int pcp_ortho_end(pcp_context *ctx) {
  if (!ctx) return PCP_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  or_drop(ctx);
  return PCP_OK;
}

}  // extern "C"

static inline bool or_project(const om::Frame &f, float x, float y, float z, int32_t *pixel, uint32_t *depth_bits) {
  return om::project(f, x, y, z, pixel, depth_bits);
}
static inline bool or_project(const cy::Frame &f, float x, float y, float z, int32_t *pixel, uint32_t *depth_bits) {
  return cy::project(f, x, y, z, pixel, depth_bits);
}

// the CPU form of a whole map under an accepted frame of either kind (pcp_ortho_host, pcp_ortho_cyl_host)
template <class FrameT>
static int or_host_map(const char *who, const FrameT &f, int64_t n, const float *xyz, const uint8_t *rgb, const uint8_t *label,
                       const uint8_t *has, int64_t index_base, int32_t fill_radius_px, uint32_t *out_index, float *out_depth,
                       uint8_t *out_rgb, uint8_t *out_label, uint8_t *out_status, int32_t *out_source, int64_t *out_contributors,
                       int64_t *out_occupied, int64_t *out_filled) {
  if (fill_radius_px < 0 || fill_radius_px > om::kMaxFill) {
    set_global_error("%s: fill radius %d outside 0..%d pixels", who, fill_radius_px, om::kMaxFill);
    return PCP_ERR_INVALID;
  }
  if (index_base < 0 || index_base > om::kMaxIndexEnd - n) {  // (index_base + n > 2^32 - 1, without the sum: it may overflow)
    set_global_error("%s: index_base %lld with %lld rows: global indices outside 0 .. 2^32 - 2", who,
                     static_cast<long long>(index_base), static_cast<long long>(n));
    return PCP_ERR_RANGE;
  }
  const int32_t w = f.w, h = f.h;
  const size_t px = static_cast<size_t>(w) * static_cast<size_t>(h);
  std::vector<unsigned long long> keys;
  std::vector<uint32_t> payload, d2;
  std::vector<int32_t> nearest;
  std::vector<uint8_t> gray;
  try {
    keys.assign(px, om::kEmptyKey);
    payload.assign(px, 0u);
    if (fill_radius_px > 0) {
      d2.resize(px);
      nearest.resize(px);
      gray.resize(px);
    }
  } catch (const std::bad_alloc &) {
    set_global_error("%s: out of host memory for %d x %d pixels", who, w, h);
    return PCP_ERR_NOMEM;
  }
  int64_t contributors = 0;
  for (int64_t i = 0; i < n; ++i) {  // OM3 and OM4 in one sequential pass: a strictly smaller key takes the pixel
    if (has && !has[i]) continue;
    int32_t pixel;
    uint32_t depth_bits;
    if (!or_project(f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &pixel, &depth_bits)) continue;
    contributors += 1;
    const unsigned long long key = om::key_of(depth_bits, static_cast<uint32_t>(index_base + i));
    if (key < keys[static_cast<size_t>(pixel)]) {
      keys[static_cast<size_t>(pixel)] = key;
      const uint32_t word = rgb[3 * i] | (static_cast<uint32_t>(rgb[3 * i + 1]) << 8) | (static_cast<uint32_t>(rgb[3 * i + 2]) << 16);
      payload[static_cast<size_t>(pixel)] = om::payload_of(word, label ? label[i] : 0u);
    }
  }
  if (fill_radius_px > 0) {  // OM6: occupied pixels are the distance transform's background
    for (size_t p = 0; p < px; ++p) gray[p] = keys[p] != om::kEmptyKey ? 0 : 255;
    const int erc = pcp_mask_edt_host(w, h, gray.data(), w, 0, d2.data(), nearest.data());
    if (erc != PCP_OK) return erc;
  }
  int64_t occupied = 0, filled = 0;
  for (size_t p = 0; p < px; ++p) {
    int32_t src;
    if (keys[p] != om::kEmptyKey) {
      src = static_cast<int32_t>(p);
      occupied += 1;
    } else {
      src = fill_radius_px > 0 ? om::fill_source(d2[p], nearest[p], fill_radius_px) : -1;
      filled += src >= 0 ? 1 : 0;
    }
    uint32_t index = om::kNoIndex, word = 0u;
    float depth = 0.0f;
    if (src >= 0) {
      index = om::key_index(keys[static_cast<size_t>(src)]);
      depth = om::key_depth(keys[static_cast<size_t>(src)]);
      word = payload[static_cast<size_t>(src)];
    }
    if (out_index) out_index[p] = index;
    if (out_depth) out_depth[p] = depth;
    if (out_rgb)
      for (int c = 0; c < 3; ++c) out_rgb[3 * p + c] = static_cast<uint8_t>(word >> (8 * c));
    if (out_label) out_label[p] = static_cast<uint8_t>(word >> 24);
    if (out_status) out_status[p] = src < 0 ? 0 : (static_cast<size_t>(src) == p ? 1 : 2);
    if (out_source) out_source[p] = src;
  }
  if (out_contributors) *out_contributors = contributors;
  if (out_occupied) *out_occupied = occupied;
  if (out_filled) *out_filled = filled;
  return PCP_OK;
}

// CY6: the closed-form cylinder of the rows that have a valid normal, and the frame that unrolls them
static int cy_fit(int64_t n, const float *xyz, const float *normal, const uint8_t *has, const double *viewer, float gsd, pcp_cyl_frame *out,
                  double *stats) {
  const char *who = "pcp_cyl_fit_host";
  auto dot = [](const double *p, const double *q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
  auto cross = [](const double *p, const double *q, double *r) {
    r[0] = p[1] * q[2] - p[2] * q[1];
    r[1] = p[2] * q[0] - p[0] * q[2];
    r[2] = p[0] * q[1] - p[1] * q[0];
  };
  // 1. the rows
  std::vector<int64_t> rows;
  try {
    for (int64_t i = 0; i < n; ++i) {
      if (has && !has[i]) continue;
      const float *p = xyz + 3 * i, *q = normal + 3 * i;
      if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2])))
        continue;
      if (q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f) continue;
      rows.push_back(i);
    }
  } catch (const std::bad_alloc &) {
    set_global_error("%s: out of host memory for %lld rows", who, static_cast<long long>(n));
    return PCP_ERR_NOMEM;
  }
  const double cnt = static_cast<double>(rows.size());
  if (rows.size() < 16) {
    set_global_error("%s: %lld rows with a valid normal, a cylinder needs 16", who, static_cast<long long>(rows.size()));
    return PCP_ERR_RANGE;
  }
  // 2. the axis: the direction the normals have least of
  double m[6] = {0, 0, 0, 0, 0, 0}, cen[3] = {0, 0, 0};
  for (const int64_t i : rows) {
    const double q[3] = {normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]};
    m[0] += q[0] * q[0];
    m[1] += q[0] * q[1];
    m[2] += q[0] * q[2];
    m[3] += q[1] * q[1];
    m[4] += q[1] * q[2];
    m[5] += q[2] * q[2];
    for (int k = 0; k < 3; ++k) cen[k] += static_cast<double>(xyz[3 * i + k]);
  }
  double scale = 0.0;
  for (int k = 0; k < 6; ++k) {
    m[k] /= cnt;
    scale = std::fmax(scale, std::fabs(m[k]));
  }
  for (int k = 0; k < 3; ++k) cen[k] /= cnt;
  double sm[6], ev[3], a[3];
  for (int k = 0; k < 6; ++k) sm[k] = m[k] / scale;
  or_roots3(sm, ev);
  if (!(ev[1] > 1e-4 * ev[2])) {
    set_global_error("%s: no direction: the normals are parallel (second eigenvalue %.3g of %.3g), a plane and not a cylinder", who,
                     ev[1] * scale, ev[2] * scale);
    return PCP_ERR_RANGE;
  }
  or_eigenvector(sm, ev[0], a);
  if (a[or_largest_component(a)] > 0.0)  // 5. rows run along +a, downwards in the picture: a's largest component is negative
    for (int k = 0; k < 3; ++k) a[k] = -a[k];
  // the fit's basis: e0 from the world axis a has least of, g0 = a x e0
  int least = 0;
  for (int k = 1; k < 3; ++k)
    if (std::fabs(a[k]) < std::fabs(a[least])) least = k;
  double e0[3], g0[3];
  for (int k = 0; k < 3; ++k) e0[k] = (k == least ? 1.0 : 0.0) - a[least] * a[k];
  const double el = std::sqrt(dot(e0, e0));
  for (int k = 0; k < 3; ++k) e0[k] /= el;
  cross(a, e0, g0);
  // 3. Kasa's circle through the rows projected along the axis, about their centroid
  double A[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  for (const int64_t i : rows) {
    const double d[3] = {xyz[3 * i] - cen[0], xyz[3 * i + 1] - cen[1], xyz[3 * i + 2] - cen[2]};
    const double u = dot(d, e0), v = dot(d, g0), z = u * u + v * v;
    A[0][0] += u * u;
    A[0][1] += u * v;
    A[0][2] += u;
    A[1][1] += v * v;
    A[1][2] += v;
    A[0][3] -= u * z;
    A[1][3] -= v * z;
    A[2][3] -= z;
  }
  A[1][0] = A[0][1];
  A[2][0] = A[0][2];
  A[2][1] = A[1][2];
  A[2][2] = cnt;
  for (int col = 0; col < 3; ++col) {  // Gaussian elimination with partial pivoting
    int piv = col;
    for (int r = col + 1; r < 3; ++r)
      if (std::fabs(A[r][col]) > std::fabs(A[piv][col])) piv = r;
    for (int k = 0; k < 4; ++k) std::swap(A[col][k], A[piv][k]);
    for (int r = col + 1; r < 3; ++r) {
      const double f = A[r][col] / A[col][col];
      for (int k = col; k < 4; ++k) A[r][k] -= f * A[col][k];
    }
  }
  double sol[3];
  for (int r = 2; r >= 0; --r) {
    double s = A[r][3];
    for (int k = r + 1; k < 3; ++k) s -= A[r][k] * sol[k];
    sol[r] = s / A[r][r];
  }
  const double uc = -0.5 * sol[0], vc = -0.5 * sol[1];
  const double R = std::sqrt(uc * uc + vc * vc - sol[2]);
  if (!(R >= static_cast<double>(cy::kMinRadius) && R <= static_cast<double>(cy::kMaxRadius))) {
    set_global_error("%s: fitted radius %.6g outside [0.05, 1000] metres", who, R);
    return PCP_ERR_RANGE;
  }
  double c0[3];
  for (int k = 0; k < 3; ++k) c0[k] = cen[k] + uc * e0[k] + vc * g0[k];
  // 4. the side: a viewer within R of the axis looks from inside
  int32_t side = -1;
  if (viewer) {
    const double w[3] = {viewer[0] - c0[0], viewer[1] - c0[1], viewer[2] - c0[2]};
    const double wa = dot(w, a);
    if (dot(w, w) - wa * wa <= R * R) side = 1;
  }
  double b0[3];
  for (int k = 0; k < 3; ++k) b0[k] = static_cast<double>(side) * g0[k];
  // 6. the seam, and the statistics
  constexpr int kBins = 4096;
  std::vector<uint8_t> occ(kBins, 0);
  const double bin_width = cy::kTwoPi / kBins, g = static_cast<double>(gsd);
  double h0 = INFINITY, h1 = -INFINITY, dev0 = INFINITY, dev1 = -INFINITY, sq = 0.0;
  for (const int64_t i : rows) {
    const double d[3] = {xyz[3 * i] - c0[0], xyz[3 * i + 1] - c0[1], xyz[3 * i + 2] - c0[2]};
    const double s = dot(d, e0), t = dot(d, b0), hh = dot(d, a);
    const double rho = std::sqrt(s * s + t * t), dev = rho - R;
    sq += dev * dev;
    dev0 = std::fmin(dev0, dev);
    dev1 = std::fmax(dev1, dev);
    h0 = std::fmin(h0, hh);
    h1 = std::fmax(h1, hh);
    if (rho > 0.0) occ[static_cast<size_t>(std::min(kBins - 1, static_cast<int>(std::floor(cy::angle(s, t) / bin_width))))] = 1;
  }
  int first = 0;
  while (first < kBins && !occ[static_cast<size_t>(first)]) ++first;
  int best = 0, best_next = 0, run = 0;
  for (int k = 1; k <= kBins && first < kBins; ++k) {  // from the lowest occupied bin once round: every run ends at an occupied bin
    const int pos = (first + k) % kBins;
    if (!occ[static_cast<size_t>(pos)]) {
      ++run;
    } else {
      if (run > best) {
        best = run;
        best_next = pos;
      }
      run = 0;
    }
  }
  const double gap = best * bin_width;
  const bool closed = gap * R < 2.0 * g;  // no room for the margins: the ring is closed and the seam stays at e0
  double e[3], b[3];
  if (closed) {
    for (int k = 0; k < 3; ++k) e[k] = e0[k];
  } else {
    const double seam = best_next * bin_width - g / R;
    const double cs = std::cos(seam), sn = std::sin(seam);
    for (int k = 0; k < 3; ++k) e[k] = cs * e0[k] + sn * b0[k];
  }
  cross(a, e, b);
  for (int k = 0; k < 3; ++k) b[k] *= static_cast<double>(side);
  // 7. the raster and the window, in the frame's own arithmetic (CY2)
  pcp_cyl_frame fr;
  bool finite = std::isfinite(h0) && std::isfinite(h1) && std::isfinite(sq);
  for (int k = 0; k < 3; ++k) {
    fr.c[k] = static_cast<float>(c0[k] + (h0 - g) * a[k]);  // one pixel above the first row
    fr.a[k] = static_cast<float>(a[k]);
    fr.e[k] = static_cast<float>(e[k]);
    fr.b[k] = static_cast<float>(b[k]);
    finite = finite && std::isfinite(fr.c[k]) && std::isfinite(fr.a[k]) && std::isfinite(fr.e[k]) && std::isfinite(fr.b[k]);
  }
  if (!finite) {
    set_global_error("%s: the fit is not finite", who);
    return PCP_ERR_RANGE;
  }
  fr.radius = static_cast<float>(R);
  fr.gsd = gsd;
  fr.side = side;
  fr.width = fr.height = 1;
  fr.d_min = 0.0f;
  fr.d_max = 1.0f;
  const cy::Frame f = or_cyl_frame(fr);
  float x1 = 0.0f, y1 = 0.0f, dlo = INFINITY, dhi = -INFINITY;
  for (const int64_t i : rows) {
    float x, y, depth;
    if (!cy::coords(f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &x, &y, &depth)) continue;
    x1 = std::fmax(x1, x);
    y1 = std::fmax(y1, y);
    dlo = std::fmin(dlo, depth);
    dhi = std::fmax(dhi, depth);
  }
  const double around = cy::kTwoPi * static_cast<double>(fr.radius);
  // (a closed ring: one column more when a row's x reaches the width, unless CY1's circumference rule forbids it -- theta
  // within a rounding of 2 pi on a wide raster: that row then lies outside the map, the stated exception to "every row")
  double wd = closed ? std::fmax(std::ceil(around / g), std::floor(static_cast<double>(x1)) + 1.0) : std::floor(static_cast<double>(x1)) + 2.0;
  if (closed && wd * g > around + g) wd = std::ceil(around / g);
  const double hd = std::floor(static_cast<double>(y1)) + 2.0;
  if (!(wd <= om::kMaxSide && hd <= om::kMaxSide && wd * hd <= static_cast<double>(om::kMaxPixels))) {
    const double fit = om::fit_gsd(closed ? around : around - gap * R, h1 - h0, 3.0);
    set_global_error("%s: %.0f x %.0f pixels at gsd %g exceed 16384 a side or 2^26 pixels; the same extent fits at gsd %.6g", who, wd, hd, g, fit);
    return PCP_ERR_RANGE;
  }
  fr.width = static_cast<int32_t>(wd);
  fr.height = static_cast<int32_t>(hd);
  fr.d_min = dlo - gsd;
  fr.d_max = dhi + gsd;
  char msg[320];
  const int rc = or_check_cyl_frame(who, &fr, msg, sizeof msg);
  if (rc != PCP_OK) {
    set_global_error("%s (the fitted frame)", msg);
    return PCP_ERR_RANGE;
  }
  *out = fr;
  if (stats) {
    stats[0] = cnt;
    stats[1] = std::sqrt(sq / cnt);
    stats[2] = dev0;
    stats[3] = dev1;
    stats[4] = cy::kTwoPi - gap;
    for (int k = 0; k < 3; ++k) stats[5 + k] = ev[k] * scale;
  }
  return PCP_OK;
}

extern "C" {

int pcp_ortho_host(const pcp_ortho_frame *frame, int64_t n, const float *xyz, const uint8_t *rgb, const uint8_t *label, const uint8_t *has,
                   int64_t index_base, int32_t fill_radius_px, uint32_t *out_index, float *out_depth, uint8_t *out_rgb, uint8_t *out_label,
                   uint8_t *out_status, int32_t *out_source, int64_t *out_contributors, int64_t *out_occupied, int64_t *out_filled) {
  if (out_contributors) *out_contributors = 0;
  if (out_occupied) *out_occupied = 0;
  if (out_filled) *out_filled = 0;
  if (!frame || n < 0 || (n > 0 && (!xyz || !rgb))) {
    set_global_error("pcp_ortho_host: NULL frame, negative n or a missing xyz / rgb");
    return PCP_ERR_INVALID;
  }
  char msg[320];
  const int rc = or_check_frame("pcp_ortho_host", frame, msg, sizeof msg);
  if (rc != PCP_OK) {
    set_global_error("%s", msg);
    return rc;
  }
  return or_host_map("pcp_ortho_host", or_frame(*frame), n, xyz, rgb, label, has, index_base, fill_radius_px, out_index, out_depth, out_rgb,
                     out_label, out_status, out_source, out_contributors, out_occupied, out_filled);
}

int pcp_ortho_cyl_host(const pcp_cyl_frame *frame, int64_t n, const float *xyz, const uint8_t *rgb, const uint8_t *label, const uint8_t *has,
                       int64_t index_base, int32_t fill_radius_px, uint32_t *out_index, float *out_depth, uint8_t *out_rgb,
                       uint8_t *out_label, uint8_t *out_status, int32_t *out_source, int64_t *out_contributors, int64_t *out_occupied,
                       int64_t *out_filled) {
  if (out_contributors) *out_contributors = 0;
  if (out_occupied) *out_occupied = 0;
  if (out_filled) *out_filled = 0;
  if (!frame || n < 0 || (n > 0 && (!xyz || !rgb))) {
    set_global_error("pcp_ortho_cyl_host: NULL frame, negative n or a missing xyz / rgb");
    return PCP_ERR_INVALID;
  }
  char msg[320];
  const int rc = or_check_cyl_frame("pcp_ortho_cyl_host", frame, msg, sizeof msg);
  if (rc != PCP_OK) {
    set_global_error("%s", msg);
    return rc;
  }
  return or_host_map("pcp_ortho_cyl_host", or_cyl_frame(*frame), n, xyz, rgb, label, has, index_base, fill_radius_px, out_index, out_depth,
                     out_rgb, out_label, out_status, out_source, out_contributors, out_occupied, out_filled);
}

int pcp_cyl_angle_host(int64_t n, const double *s, const double *t, double *out_theta) {
  if (n < 0 || (n > 0 && (!s || !t || !out_theta))) {
    set_global_error("pcp_cyl_angle_host: negative n or a NULL array");
    return PCP_ERR_INVALID;
  }
  for (int64_t i = 0; i < n; ++i) out_theta[i] = cy::angle(s[i], t[i]);
  return PCP_OK;
}

int pcp_cyl_fit_host(int64_t n, const float *xyz, const float *normal, const uint8_t *has, const double *viewer, float gsd,
                     pcp_cyl_frame *out, double out_stats[8]) {
  if (n < 0 || (n > 0 && (!xyz || !normal)) || !out) {
    set_global_error("pcp_cyl_fit_host: negative n, NULL xyz, NULL normal or NULL frame");
    return PCP_ERR_INVALID;
  }
  if (!(std::isfinite(gsd) && gsd >= 1e-4f && gsd <= 1.0f)) {
    set_global_error("pcp_cyl_fit_host: gsd %g outside [1e-4, 1]", static_cast<double>(gsd));
    return PCP_ERR_INVALID;
  }
  if (viewer && !(std::isfinite(viewer[0]) && std::isfinite(viewer[1]) && std::isfinite(viewer[2]))) {
    set_global_error("pcp_cyl_fit_host: the viewer is not finite");
    return PCP_ERR_INVALID;
  }
  return cy_fit(n, xyz, normal, has, viewer, gsd, out, out_stats);
}

int pcp_ortho_fit_frame_host(int64_t n, const float *xyz, const uint8_t *has, const double *viewer, float gsd, pcp_ortho_frame *out) {
  if (n < 0 || (n > 0 && !xyz) || !out) {
    set_global_error("pcp_ortho_fit_frame_host: negative n, NULL xyz or NULL frame");
    return PCP_ERR_INVALID;
  }
  if (!(std::isfinite(gsd) && gsd >= 1e-4f && gsd <= 1.0f)) {
    set_global_error("pcp_ortho_fit_frame_host: gsd %g outside [1e-4, 1]", static_cast<double>(gsd));
    return PCP_ERR_INVALID;
  }
  // centroid, then the covariance about it
  int64_t rows = 0;
  double c[3] = {0.0, 0.0, 0.0};
  for (int64_t i = 0; i < n; ++i) {
    if (has && !has[i]) continue;
    rows += 1;
    for (int a = 0; a < 3; ++a) c[a] += static_cast<double>(xyz[3 * i + a]);
  }
  if (rows < 3) {
    set_global_error("pcp_ortho_fit_frame_host: %lld rows, a plane needs 3", static_cast<long long>(rows));
    return PCP_ERR_INVALID;
  }
  for (int a = 0; a < 3; ++a) c[a] /= static_cast<double>(rows);
  double m[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = 0; i < n; ++i) {
    if (has && !has[i]) continue;
    const double d[3] = {xyz[3 * i] - c[0], xyz[3 * i + 1] - c[1], xyz[3 * i + 2] - c[2]};
    m[0] += d[0] * d[0];
    m[1] += d[0] * d[1];
    m[2] += d[0] * d[2];
    m[3] += d[1] * d[1];
    m[4] += d[1] * d[2];
    m[5] += d[2] * d[2];
  }
  double scale = 0.0;
  for (int k = 0; k < 6; ++k) {
    m[k] /= static_cast<double>(rows);
    scale = std::fmax(scale, std::fabs(m[k]));
  }
  if (!(scale > DBL_MIN)) scale = 1.0;  // (also takes a NaN on to the finite check below)
  double a[6], r[3], nn[3], uu[3];
  for (int k = 0; k < 6; ++k) a[k] = m[k] / scale;
  or_roots3(a, r);
  or_eigenvector(a, r[0], nn);
  or_eigenvector(a, r[2], uu);
  // signs: the viewer in front of the plane (negative depth), else n's largest component negative; u's largest positive
  bool flip;
  if (viewer)
    flip = ((viewer[0] - c[0]) * nn[0] + (viewer[1] - c[1]) * nn[1]) + (viewer[2] - c[2]) * nn[2] > 0.0;
  else
    flip = nn[or_largest_component(nn)] > 0.0;
  if (flip)
    for (int k = 0; k < 3; ++k) nn[k] = -nn[k];
  // (u made exactly orthogonal to n: the two closed-form vectors agree to rounding only)
  const double un = uu[0] * nn[0] + uu[1] * nn[1] + uu[2] * nn[2];
  for (int k = 0; k < 3; ++k) uu[k] -= un * nn[k];
  const double ul = std::sqrt(uu[0] * uu[0] + uu[1] * uu[1] + uu[2] * uu[2]);
  for (int k = 0; k < 3; ++k) uu[k] /= ul;
  if (uu[or_largest_component(uu)] < 0.0)
    for (int k = 0; k < 3; ++k) uu[k] = -uu[k];
  const double vv[3] = {nn[1] * uu[2] - nn[2] * uu[1], nn[2] * uu[0] - nn[0] * uu[2], nn[0] * uu[1] - nn[1] * uu[0]};
  // the rows' bounding rectangle on the plane through the centroid
  double s0 = INFINITY, s1 = -INFINITY, t0 = INFINITY, t1 = -INFINITY;
  for (int64_t i = 0; i < n; ++i) {
    if (has && !has[i]) continue;
    const double d[3] = {xyz[3 * i] - c[0], xyz[3 * i + 1] - c[1], xyz[3 * i + 2] - c[2]};
    const double s = d[0] * uu[0] + d[1] * uu[1] + d[2] * uu[2], t = d[0] * vv[0] + d[1] * vv[1] + d[2] * vv[2];
    s0 = std::fmin(s0, s);
    s1 = std::fmax(s1, s);
    t0 = std::fmin(t0, t);
    t1 = std::fmax(t1, t);
  }
  const double g = static_cast<double>(gsd);
  pcp_ortho_frame fr;
  bool finite = std::isfinite(s0) && std::isfinite(s1) && std::isfinite(t0) && std::isfinite(t1);
  for (int k = 0; k < 3; ++k) {
    fr.o[k] = static_cast<float>(c[k] + (s0 - g) * uu[k] + (t0 - g) * vv[k]);  // one pixel outside the rectangle
    fr.u[k] = static_cast<float>(uu[k]);
    fr.v[k] = static_cast<float>(vv[k]);
    fr.n[k] = static_cast<float>(nn[k]);
    finite = finite && std::isfinite(fr.o[k]) && std::isfinite(fr.u[k]) && std::isfinite(fr.v[k]) && std::isfinite(fr.n[k]);
  }
  if (!finite) {
    set_global_error("pcp_ortho_fit_frame_host: the fit is not finite (a non-finite row, or rows that span no plane)");
    return PCP_ERR_INVALID;
  }
  fr.gsd = gsd;
  const double wd = std::floor((s1 - s0) / g) + 3.0, hd = std::floor((t1 - t0) / g) + 3.0;  // the rectangle plus two pixels
  if (wd > om::kMaxSide || hd > om::kMaxSide || wd * hd > static_cast<double>(om::kMaxPixels)) {
    const double fit = om::fit_gsd(s1 - s0, t1 - t0, 3.0);
    set_global_error("pcp_ortho_fit_frame_host: %.0f x %.0f pixels at gsd %g exceed 16384 a side or 2^26 pixels; the same extent fits at gsd %.6g",
                     wd, hd, g, fit);
    return PCP_ERR_RANGE;
  }
  fr.width = static_cast<int32_t>(wd);
  fr.height = static_cast<int32_t>(hd);
  // the depth window: the rows' range in the frame's own fp32 arithmetic (OM2), widened by one gsd
  om::Frame f = or_frame(fr);
  float dlo = INFINITY, dhi = -INFINITY;
  for (int64_t i = 0; i < n; ++i) {
    if (has && !has[i]) continue;
    const float d[3] = {xyz[3 * i] - f.o[0], xyz[3 * i + 1] - f.o[1], xyz[3 * i + 2] - f.o[2]};
    const float depth = om::dot3(d, f.n);
    dlo = std::fmin(dlo, depth);
    dhi = std::fmax(dhi, depth);
  }
  fr.d_min = dlo - gsd;
  fr.d_max = dhi + gsd;
  if (!(std::isfinite(fr.d_min) && std::isfinite(fr.d_max))) {
    set_global_error("pcp_ortho_fit_frame_host: the depth range is not finite");
    return PCP_ERR_INVALID;
  }
  *out = fr;
  return PCP_OK;
}

}  // extern "C"
