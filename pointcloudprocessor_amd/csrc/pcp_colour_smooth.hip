// pcp_colour_smooth.hip -- PointCloudProcessor::smoothColorsWithLocalRegion (PCP/src/PointCloudProcessor.cpp:634-703; its
// call, smoothColorsWithLocalRegion(rgbCloud, 0.1), is commented out at :597) on gfx950, as an opt-in post-pass over the
// packed colour words of the whole map.  The rules are DESIGN.md LS1-LS7:
//   - the finite points are both the queries and the candidates (LS1); non-finite points keep their word;
//   - j is a neighbour of i iff fl32 d2 = ((dx*dx + dy*dy) + dz*dz) <= t, t = the largest float with (double)t <= (double)r^2
//     -- the same decision as (double)d2 <= (double)r * (double)r (LS2);
//   - w = fl32(1 / fl32(1 + d2)) (LS3), an IEEE quotient (-fhip-fp32-correctly-rounded-divide-sqrt);
//   - out_c = floor(sum m_j c_j / sum m_j) with m_j = w_j * 2^24, an integer (w_j in [0.5, 1] for r <= 1): both sums are
//     exact 64-bit integer sums, so the result does not depend on the order of the neighbours (LS4);
//   - every output reads the unsmoothed words (LS5); has = (r | g | b) != 0 afterwards (LS6).
//
// Search: the cell-wave search of pcp_cell_search.hpp over the finite points, the record's word the unsmoothed colour word.
// Results are stored in the caller's order.
#include <algorithm>
#include <cmath>

#include "pcp_cell_search.hpp"
#include "pcp_internal.hpp"

namespace pcp {

// the record's word is the unsmoothed colour word; dst[k] = the caller's index the result of place k goes to
struct LsStage {
  const int32_t *remap;
  const uint32_t *words;
  int32_t *dst;
  __device__ uint32_t word(int64_t k, int32_t v) const {
    const int32_t i = remap[v];
    dst[k] = i;
    return words[i];
  }
  __device__ bool opens(uint32_t) const { return true; }
};

// one work item: the queries k0 .. k0 + n - 1 of one cell against the records of the neighbouring cells
__global__ __launch_bounds__(kCellQ) void k_ls_smooth(const uint4 *__restrict__ rec, const int32_t *__restrict__ dst,
                                                      const int32_t *__restrict__ items, GridDesc g,
                                                      const int32_t *__restrict__ start, float t, uint32_t *__restrict__ out) {
  const CellItem it = cell_open(rec, items, g, start);
  const int lane = threadIdx.x;
  const bool active = lane < it.n;
  const float qx = __uint_as_float(it.q.x), qy = __uint_as_float(it.q.y), qz = __uint_as_float(it.q.z);
  // m_j <= 2^24 and c_j <= 255: every product fits 32 bits, the sums stay below 2^63 for fewer than 2^31 points
  uint64_t sm = 0, sr = 0, sg = 0, sb = 0;
  cell_walk(rec, g, start, it, active, [&](const uint4 &c) {
    const float dx = __uint_as_float(c.x) - qx, dy = __uint_as_float(c.y) - qy, dz = __uint_as_float(c.z) - qz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;  // every operation rounded on its own (-ffp-contract=off)
    if (d2 <= t) {
      const float w = 1.0f / (1.0f + d2);
      const uint32_t mw = static_cast<uint32_t>(w * 16777216.0f);  // exact: w is a multiple of 2^-24 in [0.5, 1]
      sm += mw;
      sr += mw * (c.w & 0xffu);
      sg += mw * ((c.w >> 8) & 0xffu);
      sb += mw * ((c.w >> 16) & 0xffu);
    }
  });
  if (!active) return;
  // sm >= 2^24: the query is its own neighbour (d2 = 0, w = 1)
  const uint32_t r = static_cast<uint32_t>(sr / sm), gg = static_cast<uint32_t>(sg / sm), bb = static_cast<uint32_t>(sb / sm);
  const uint32_t has = (r | gg | bb) != 0u ? 1u : 0u;
  out[dst[it.k0 + lane]] = r | (gg << 8) | (bb << 16) | (has << 24);
}

// words with the has bit set: a grid-stride loop, one atomic per workgroup (one per wavefront on a single address
// queued up in its L2 channel: 1.9 ms for 10 M words)
constexpr uint32_t kLsCountBlocks = 1024;
__global__ __launch_bounds__(kCellBlock) void k_ls_count_has(const uint32_t *__restrict__ words, int64_t n,
                                                             unsigned long long *__restrict__ count) {
  __shared__ uint32_t part[kCellBlock / 64];
  uint32_t c = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kCellBlock)
    c += (words[i] >> 24) & 1u;
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < kCellBlock / 64; ++w) t += part[w];
    if (t) atomicAdd(count, t);
  }
}

// per-call scratch: released when the call returns (a 10 M-point map holds ~300 MB of it)
struct LsScratch {
  FiniteScratch fin;  // (its flags serve the work items once the view is gathered)
  CellSearch search;
  DevBuf<int32_t> dst;
};

// the m > 0 finite points of view cv: the search's records and work items, the smoothing pass into d_out
static int smooth_finite(pcp_context *ctx, const CloudView &cv, float radius, float t, const uint32_t *d_in, uint32_t *d_out,
                         LsScratch &s) {
  const int64_t m = cv.n;
  CellSearch &cs = s.search;
  PCP_HIP_TRY(ctx, s.dst.ensure(static_cast<size_t>(m) + 4));
  int rc = cell_search_prepare(ctx, cv, radius, "local colour smoothing", PCP_K_COLOUR_SMOOTH, LsStage{cv.remap, d_in, s.dst.p}, m,
                               s.fin.flag, cs);
  if (rc != PCP_OK) return rc;
  {
    LaunchTimer lt(ctx, PCP_K_COLOUR_SMOOTH);
    if (cs.n_items > 0)
      hipLaunchKernelGGL(k_ls_smooth, dim3(static_cast<uint32_t>(cs.n_items)), dim3(kCellQ), 0, ctx->stream, cs.rec.p, s.dst.p,
                         cs.items.p, cs.g, ctx->g_start.p, t, d_out);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return PCP_OK;
}

bool smooth_radius_ok(float radius) { return std::isfinite(radius) && radius > 0.0f && radius <= 1.0f; }

int colour_smooth_words(pcp_context *ctx, float radius, const uint32_t *d_in, uint32_t *d_out, int64_t *out_has_count) {
  const int64_t n = ctx->n;
  if (out_has_count) *out_has_count = 0;
  if (n == 0) return PCP_OK;
  if (d_in != d_out)  // the non-finite points keep their word; the finite ones are all overwritten below
    PCP_HIP_TRY(ctx, hipMemcpyAsync(d_out, d_in, static_cast<size_t>(n) * 4, hipMemcpyDeviceToDevice, ctx->stream));
  // LS2: (double)d2 <= (double)r * (double)r  <=>  d2 <= t for every float d2
  const double r2 = static_cast<double>(radius) * static_cast<double>(radius);
  float t = static_cast<float>(r2);
  if (static_cast<double>(t) > r2) t = std::nextafter(t, 0.0f);
  LsScratch s;
  CloudView cv;
  // LS1: the grid (which needs finite coordinates) is built over the finite points only
  int rc = finite_view(ctx, /*with_remap=*/true, /*timing_slot=*/-1, s.fin, &cv);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, ctx->s_counter.ensure(4));
  if (cv.n > 0 && (rc = smooth_finite(ctx, cv, radius, t, d_in, d_out, s)) != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->s_counter.p, 0, 8, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_COLOUR_SMOOTH);
    hipLaunchKernelGGL(k_ls_count_has, dim3(std::min(cell_blocks(n), kLsCountBlocks)), dim3(kCellBlock), 0, ctx->stream, d_out, n,
                       ctx->s_counter.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  unsigned long long c = 0;
  PCP_HIP_TRY(ctx, hipMemcpyAsync(&c, ctx->s_counter.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (also: the scratch is released on return)
  if (out_has_count) *out_has_count = static_cast<int64_t>(c);
  drop_large_grid_bitmap(ctx);  // (a tiny radius on a large map may take the sparse grid)
  return PCP_OK;
}

// (pcp_create loads every code object of the library up front: see preload_code_objects in pcp_context.hip)
hipError_t preload_colour_smooth() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_ls_smooth));
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_colour_smooth_local_packed(pcp_context *ctx, float radius, const uint32_t *in_rgba, uint32_t *out_rgba,
                                   int64_t *out_has_count) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!smooth_radius_ok(radius))
    return set_error(ctx, PCP_ERR_INVALID, "pcp_colour_smooth_local_packed: radius %g outside (0, 1]", static_cast<double>(radius));
  if (!ctx->xyz.p && ctx->n > 0) return set_error(ctx, PCP_ERR_STATE, "pcp_colour_smooth_local_packed: no cloud uploaded");
  if (out_has_count) *out_has_count = 0;
  const int64_t n = ctx->n;
  if (n == 0) return PCP_OK;
  if (!in_rgba || !out_rgba) return set_error(ctx, PCP_ERR_INVALID, "pcp_colour_smooth_local_packed: NULL words");
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevBuf<uint32_t> words;  // the caller's words (host or device memory; in == out allowed)
  PCP_HIP_TRY(ctx, words.ensure(static_cast<size_t>(n) + 4));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(words.p, in_rgba, static_cast<size_t>(n) * 4, hipMemcpyDefault, ctx->stream));
  int rc = colour_smooth_words(ctx, radius, words.p, words.p, out_has_count);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rgba, words.p, static_cast<size_t>(n) * 4, hipMemcpyDefault, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

}  // extern "C"
