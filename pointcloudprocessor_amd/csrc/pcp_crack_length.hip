// pcp_crack_length.hip -- crack lengths on the map ("Crack lengths on the map", CL1-CL9): per crack of
// pcp_crack_components a geodesic length, its two ends and an ordered polyline through it, per crack point its arc position.
// The reference's script orders a crack only by a 2-D skeleton per keyframe (scripts/genNormAndDistanceMask.py :396-478).
//
// The stage runs after the component stage for its parameters (crack_map_run, pcp_crack_fuse.hip) on that call's
// scratch: the crack points in cell order, the grid, the roots and their ranks.  Everything here is indexed by the PLACE of a
// crack point in the cell order, so that the neighbours a lane visits lie next to each other in every array.
// Two sweeps (from the label of every crack, then from the farthest point found) are label-correcting relaxations with
// integer weights: one launch is one round over the places whose distance fell in the round before, distances fall by 64-bit
// atomicMin, a lowered place is marked with the round's number, and the host reads one word per round.  No lane waits for
// another one and no kernel loops on a word that another workgroup writes.  The ends are ordered maxima in two steps, the
// predecessors one lane per place after the second sweep has ended, the paths one lane per crack (count, scan, fill).
#include <algorithm>
#include <new>
#include <vector>

#include "pcp_device.hpp"
#include "pcp_crack_map.hpp"
#include "pcp_scan.hpp"
#include "pcp_crack_length.hpp"

namespace pcp {

constexpr int kClBlock = 256;

static inline uint32_t cl_blocks(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kClBlock))); }

// CL8: words that other lanes may lower or raise in the same kernel are read at agent scope (the L2s of the XCDs are not
// coherent for plain accesses; CC5)
__device__ __forceinline__ unsigned long long cl_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t cl_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// place s holds view index order[s]: its inverse, the row of every place and the place of every crack's label
__global__ __launch_bounds__(kClBlock) void k_cl_rows(const int32_t *__restrict__ order, const int32_t *__restrict__ root_of,
                                                      const int32_t *__restrict__ rank, int64_t m, int32_t *__restrict__ place_of,
                                                      int32_t *__restrict__ row_of, int32_t *__restrict__ src_place) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  if (s >= m) return;
  const int32_t k = order[s];
  const int32_t root = root_of[k];
  const int32_t row = rank[root];
  place_of[k] = static_cast<int32_t>(s);
  row_of[s] = row;
  if (root == k) src_place[row] = static_cast<int32_t>(s);
}

__global__ __launch_bounds__(kClBlock) void k_cl_clear(unsigned long long *__restrict__ dist, int64_t m) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  if (s < m) dist[s] = cl::kNoPos;
}

// the sources of a sweep, one per crack, marked as lowered in round `round`; and the empty ordered maximum of every crack
__global__ __launch_bounds__(kClBlock) void k_cl_seed(const int32_t *__restrict__ src_place, int64_t rows, uint32_t round,
                                                      unsigned long long *__restrict__ dist, uint32_t *__restrict__ mark,
                                                      unsigned long long *__restrict__ far_d, int32_t *__restrict__ far_k) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  if (r >= rows) return;
  const int32_t s = src_place[r];
  dist[s] = 0;
  mark[s] = round;
  far_d[r] = 0;
  far_k[r] = 0x7fffffff;
}

// CL8, one round: a lane per place; the places marked in the round before (or already in this one) relax every link they
// have, to earlier and later places alike.  mark words never exceed `round`, and *fell is raised to `round` iff some
// distance fell.
__global__ __launch_bounds__(kClBlock) void k_cl_relax(const float *__restrict__ gx, const float *__restrict__ gy,
                                                       const float *__restrict__ gz, int64_t m, GridDesc g,
                                                       const int32_t *__restrict__ start, float t, uint32_t round,
                                                       unsigned long long *__restrict__ dist, uint32_t *__restrict__ mark,
                                                       uint32_t *__restrict__ fell) {
  const int64_t s64 = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  bool lowered = false;
  if (s64 < m && cl_load(mark + s64) + 1u >= round) {
    const int32_t s = static_cast<int32_t>(s64);
    const unsigned long long ds = cl_load(dist + s);
    const float qx = gx[s], qy = gy[s], qz = gz[s];
    crack_walk<false>(g, start, qx, qy, qz, s, m, [&](int32_t c) {
      const float d2 = cl::d2_of(gx[c] - qx, gy[c] - qy, gz[c] - qz);
      if (!(d2 <= t)) return;
      const unsigned long long dc = cl_load(dist + c);
      if (ds + 1 >= dc) return;  // every weight is at least 1: nothing to lower, and no square root to take
      const unsigned long long nd = ds + cl::weight(d2);
      if (nd >= dc) return;
      if (atomicMin(dist + c, nd) > nd) {
        atomicMax(mark + c, round);
        lowered = true;
      }
    });
  }
  if (__ballot(lowered) && (threadIdx.x & 63) == 0) atomicMax(fell, round);
}

// CL4, step 1: the largest distance of every crack
__global__ __launch_bounds__(kClBlock) void k_cl_far_d(const unsigned long long *__restrict__ dist, const int32_t *__restrict__ row_of,
                                                       int64_t m, unsigned long long *__restrict__ far_d) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  if (s >= m) return;
  const unsigned long long d = dist[s];
  unsigned long long *w = far_d + row_of[s];
  if (d > cl_load(w)) atomicMax(w, d);
}

// CL4, step 2: the lowest index among the points that hold it (view indices ascend as the input indices do)
__global__ __launch_bounds__(kClBlock) void k_cl_far_k(const unsigned long long *__restrict__ dist, const int32_t *__restrict__ row_of,
                                                       const int32_t *__restrict__ order, int64_t m,
                                                       const unsigned long long *__restrict__ far_d, int32_t *__restrict__ far_k) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  if (s >= m) return;
  const int32_t row = row_of[s];
  if (dist[s] == far_d[row]) atomicMin(far_k + row, order[s]);
}

// the end of every crack (view index) kept, and its place as the source of the next sweep
__global__ __launch_bounds__(kClBlock) void k_cl_end(const int32_t *__restrict__ far_k, const int32_t *__restrict__ place_of, int64_t rows,
                                                     int64_t m, int32_t *__restrict__ end_k, int32_t *__restrict__ src_place,
                                                     uint32_t *__restrict__ bad) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  if (r >= rows) return;
  int32_t k = far_k[r];
  if (k < 0 || k >= m) {  // (cannot be: every crack has a point at its largest distance)
    atomicMax(bad, 1u);
    k = 0;
  }
  end_k[r] = k;
  src_place[r] = place_of[k];
}

// CL6, after the second sweep has ended: plain loads.  pred[s] = the place of the predecessor, -1 for the end a itself.
__global__ __launch_bounds__(kClBlock) void k_cl_pred(const float *__restrict__ gx, const float *__restrict__ gy,
                                                      const float *__restrict__ gz, const int32_t *__restrict__ order, int64_t m,
                                                      GridDesc g, const int32_t *__restrict__ start, float t,
                                                      const unsigned long long *__restrict__ dist, int32_t *__restrict__ pred) {
  const int64_t s64 = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  if (s64 >= m) return;
  const int32_t s = static_cast<int32_t>(s64);
  const unsigned long long ds = dist[s];
  int32_t best_k = -1, best_place = -1;
  if (ds != 0) {
    const float qx = gx[s], qy = gy[s], qz = gz[s];
    crack_walk<false>(g, start, qx, qy, qz, s, m, [&](int32_t c) {
      const float d2 = cl::d2_of(gx[c] - qx, gy[c] - qy, gz[c] - qz);
      if (!(d2 <= t) || !cl::pred_ok(dist[c], cl::weight(d2), ds)) return;
      const int32_t k = order[c];
      if (cl::pred_better(k, best_k)) {
        best_k = k;
        best_place = c;
      }
    });
  }
  pred[s] = best_place;
}

// CL8: one lane per crack walks from b to a.  fill == false: counts[r] = hops + 1.  fill == true: the path from a to b, the
// three statistics of the fused w along it and the row of the table.  The loop is bounded by the crack's point count.
template <bool fill>
__global__ __launch_bounds__(kClBlock) void k_cl_walk(const int32_t *__restrict__ end_a, const int32_t *__restrict__ end_b,
                                                      const int32_t *__restrict__ place_of, const int32_t *__restrict__ pred,
                                                      const unsigned long long *__restrict__ cc_stats, int64_t rows, int64_t m,
                                                      int32_t *__restrict__ counts, const int32_t *__restrict__ order,
                                                      const int32_t *__restrict__ list, const unsigned long long *__restrict__ dist,
                                                      int64_t n, const uint32_t *__restrict__ u32, const unsigned long long *__restrict__ u64,
                                                      int32_t *__restrict__ path, long long *__restrict__ table, uint32_t *__restrict__ bad) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  if (r >= rows) return;
  const long long points = static_cast<long long>(min(cc_stats[kCcStatWords * r]  /* word 0: points */, static_cast<unsigned long long>(m)));
  int32_t s = place_of[end_b[r]];
  if (!fill) {
    long long hops = 0;
    while (pred[s] >= 0 && hops < points) {
      s = pred[s];
      ++hops;
    }
    if (pred[s] >= 0 || hops >= points) {  // (cannot be: D strictly decreases along pred)
      atomicMax(bad, 1u);
      hops = 0;
    }
    counts[r] = static_cast<int32_t>(hops + 1);
    return;
  }
  const long long off = counts[r], len = static_cast<long long>(counts[r + 1]) - off;  // (scanned: offsets)
  unsigned long long sum_w = 0, min_w = ~0ull, max_w = 0;
  const unsigned long long length_q = dist[s];
  for (long long c = 0; c < len; ++c) {
    const int32_t i = list[order[s]];
    path[off + (len - 1 - c)] = i;
    const unsigned long long w = cf::fused_w(u64[i], u32[n + i]);
    sum_w += w;
    min_w = min(min_w, w);
    max_w = max(max_w, w);
    const int32_t p = pred[s];
    if (p < 0) break;
    s = p;
  }
  long long *row = table + static_cast<int64_t>(cl::kRowWords) * r;
  row[0] = list[end_a[r]];
  row[1] = list[end_b[r]];
  row[2] = static_cast<long long>(length_q);
  row[3] = len - 1;
  row[4] = static_cast<long long>(sum_w);
  row[5] = static_cast<long long>(min_w);
  row[6] = static_cast<long long>(max_w);
}

// CL5 (the other points keep the 2^64 - 1 the buffer was filled with)
__global__ __launch_bounds__(kClBlock) void k_cl_pos(const unsigned long long *__restrict__ dist, const int32_t *__restrict__ order,
                                                     const int32_t *__restrict__ list, int64_t m, unsigned long long *__restrict__ pos) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kClBlock + threadIdx.x;
  if (s < m) pos[list[order[s]]] = dist[s];
}

hipError_t preload_crack_length() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_cl_relax));
}

// one sweep from src_place: rounds until nothing falls; *round counts on through both sweeps, so that no mark of the first
// sweep can be mistaken for one of the second
static int sweep(pcp_context *ctx, const CcScratch &cc, ClScratch &s, int64_t m, int64_t rows, float t, uint32_t *round) {
  const size_t pm = (static_cast<size_t>(m) + 3) & ~size_t(3);
  const float *gx = ctx->g_xyz.p, *gy = ctx->g_xyz.p + pm, *gz = ctx->g_xyz.p + 2 * pm;
  *round += 1;
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cl_clear, dim3(cl_blocks(m)), dim3(kClBlock), 0, ctx->stream, s.dist.p, m);
    hipLaunchKernelGGL(k_cl_seed, dim3(cl_blocks(rows)), dim3(kClBlock), 0, ctx->stream, s.src_place.p, rows, *round, s.dist.p, s.mark.p,
                       s.far_d.p, s.far_k.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  // CL8: after round k every point whose shortest path has at most k links is final, and no shortest path has m links
  int64_t k = 0;
  for (; k <= m; ++k) {
    *round += 1;
    {
      LaunchTimer lt(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_cl_relax, dim3(cl_blocks(m)), dim3(kClBlock), 0, ctx->stream, gx, gy, gz, m, cc.grid, ctx->g_start.p, t, *round,
                         s.dist.p, s.mark.p, s.words.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    uint32_t fell = 0;
    PCP_HIP_TRY(ctx, hipMemcpyAsync(&fell, s.words.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (fell != *round) break;
  }
  if (k > m) return set_error(ctx, PCP_ERR_DEVICE, "pcp_crack_lengths: a sweep over %lld crack points did not settle in %lld rounds", (long long)m, (long long)(m + 1));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cl_far_d, dim3(cl_blocks(m)), dim3(kClBlock), 0, ctx->stream, s.dist.p, s.row_of.p, m, s.far_d.p);
    hipLaunchKernelGGL(k_cl_far_k, dim3(cl_blocks(m)), dim3(kClBlock), 0, ctx->stream, s.dist.p, s.row_of.p, ctx->g_order.p, m, s.far_d.p,
                       s.far_k.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return PCP_OK;
}

// the m > 0 crack points and rows > 0 cracks the component stage left in cc and ctx->g_*; CL5 into s.pos where the caller made it
int crack_lengths_run(pcp_context *ctx, const pcp_crack_link_params &p, const CcScratch &cc, ClScratch &s, CrackCounts *c) {
  CrackMap &cm = *ctx->crack;
  const int64_t m = c->points, rows = c->cracks;
  const size_t sm = static_cast<size_t>(m), sr = static_cast<size_t>(rows);
  const size_t pm = (sm + 3) & ~size_t(3);
  const float *gx = ctx->g_xyz.p, *gy = ctx->g_xyz.p + pm, *gz = ctx->g_xyz.p + 2 * pm;
  const float t = gn::threshold_of(p.radius);
  if (2 * static_cast<uint64_t>(m) + 8 > 0xffffffffull) return set_error(ctx, PCP_ERR_INVALID, "pcp_crack_lengths: %lld crack points are too many", (long long)m);
  PCP_HIP_TRY(ctx, s.dist.ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.mark.ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.words.ensure(4));
  PCP_HIP_TRY(ctx, s.place_of.ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.row_of.ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.pred.ensure(sm + 4));
  PCP_HIP_TRY(ctx, s.far_d.ensure(sr + 4));
  for (DevBuf<int32_t> *b : {&s.src_place, &s.far_k, &s.end_a, &s.end_b}) PCP_HIP_TRY(ctx, b->ensure(sr + 4));
  PCP_HIP_TRY(ctx, cm.cl_ids.ensure(sr + 4));
  PCP_HIP_TRY(ctx, cm.cl_offsets.ensure(sr + 8));
  PCP_HIP_TRY(ctx, cm.cl_table.ensure(static_cast<size_t>(cl::kRowWords) * sr + 4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.mark.p, 0, sm * 4, ctx->stream));  // round 0: before every round of this call
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.words.p, 0, 16, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(cm.cl_ids.p, cm.cc_ids.p, sr * 4, hipMemcpyDeviceToDevice, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cl_rows, dim3(cl_blocks(m)), dim3(kClBlock), 0, ctx->stream, ctx->g_order.p, cc.root_of.p, cc.rank.p, m, s.place_of.p,
                       s.row_of.p, s.src_place.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  uint32_t round = 0;
  int rc = sweep(ctx, cc, s, m, rows, t, &round);  // CL4: from s0 ...
  if (rc != PCP_OK) return rc;
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cl_end, dim3(cl_blocks(rows)), dim3(kClBlock), 0, ctx->stream, s.far_k.p, s.place_of.p, rows, m, s.end_a.p,
                       s.src_place.p, s.words.p + 1);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  if ((rc = sweep(ctx, cc, s, m, rows, t, &round)) != PCP_OK) return rc;  // ... and from a
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cl_end, dim3(cl_blocks(rows)), dim3(kClBlock), 0, ctx->stream, s.far_k.p, s.place_of.p, rows, m, s.end_b.p,
                       s.src_place.p, s.words.p + 1);
    hipLaunchKernelGGL(k_cl_pred, dim3(cl_blocks(m)), dim3(kClBlock), 0, ctx->stream, gx, gy, gz, ctx->g_order.p, m, cc.grid, ctx->g_start.p, t,
                       s.dist.p, s.pred.p);
    PCP_HIP_TRY(ctx, hipMemsetAsync(cm.cl_offsets.p, 0, (sr + 8) * 4, ctx->stream));
    hipLaunchKernelGGL(k_cl_walk<false>, dim3(cl_blocks(rows)), dim3(kClBlock), 0, ctx->stream, s.end_a.p, s.end_b.p, s.place_of.p, s.pred.p,
                       cm.cc_stats.p, rows, m, cm.cl_offsets.p, nullptr, nullptr, nullptr, ctx->n, nullptr, nullptr, nullptr, nullptr,
                       s.words.p + 1);
    PCP_HIP_TRY(ctx, hipGetLastError());
    PCP_HIP_TRY(ctx, scan_exclusive(ctx->stream, cm.cl_offsets.p, rows + 1, ctx->s_tiles, nullptr));  // [rows] = all entries
  }
  int32_t entries = 0;
  uint32_t bad = 0;
  PCP_HIP_TRY(ctx, hipMemcpyAsync(&entries, cm.cl_offsets.p + rows, 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(&bad, s.words.p + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (bad || entries < rows || entries > m)
    return set_error(ctx, PCP_ERR_DEVICE, "pcp_crack_lengths: %d path entries for %lld cracks of %lld points (flag %u)", entries, (long long)rows, (long long)m, bad);
  PCP_HIP_TRY(ctx, cm.cl_path.ensure(static_cast<size_t>(entries) + 4));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cl_walk<true>, dim3(cl_blocks(rows)), dim3(kClBlock), 0, ctx->stream, s.end_a.p, s.end_b.p, s.place_of.p, s.pred.p,
                       cm.cc_stats.p, rows, m, cm.cl_offsets.p, ctx->g_order.p, cc.list.p, s.dist.p, ctx->n, cm.cf_u32.p, cm.cf_u64.p,
                       cm.cl_path.p, cm.cl_table.p, s.words.p + 1);
    if (s.pos.p) hipLaunchKernelGGL(k_cl_pos, dim3(cl_blocks(m)), dim3(kClBlock), 0, ctx->stream, s.dist.p, ctx->g_order.p, cc.list.p, m, s.pos.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  c->entries = entries;
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_crack_lengths(pcp_context *ctx, const pcp_crack_link_params *p, uint64_t *out_pos, int64_t *out_cracks, int64_t *out_path_points) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_cracks) *out_cracks = 0;
  if (out_path_points) *out_path_points = 0;
  int rc = crack_link_check(ctx, "pcp_crack_lengths", p);
  if (rc != PCP_OK) return rc;
  CrackOut out;
  out.pos = out_pos;
  CrackCounts c;
  if ((rc = crack_map_run(ctx, *p, CrackMap::kLengths, 0, out, &c)) != PCP_OK) return rc;
  if (out_cracks) *out_cracks = c.cracks;
  if (out_path_points) *out_path_points = c.entries;
  return PCP_OK;
}

int pcp_crack_lengths_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows7, int64_t *out_offsets,
                            int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  const CrackMap &cm = *ctx->crack;
  int64_t rows = 0;
  const int rc = crack_window(ctx, "pcp_crack_lengths_fetch", CrackMap::kLengths, first, max_rows, cm.cl_rows, &rows);
  if (rc != PCP_OK) return rc;
  if (rows == 0) {  // no row: entry 0 is still where row `first` starts (the end of the paths from the last row on)
    if (out_offsets) {
      int32_t at = 0;
      if (first < cm.cl_rows) {
        PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        PCP_HIP_TRY(ctx, hipMemcpyAsync(&at, cm.cl_offsets.p + first, 4, hipMemcpyDeviceToHost, ctx->stream));
        PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      }
      out_offsets[0] = first < cm.cl_rows ? at : cm.cl_entries;
    }
    return PCP_OK;
  }
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t sr = static_cast<size_t>(rows), sf = static_cast<size_t>(first);
  std::vector<int32_t> off;
  try {
    if (out_offsets) off.resize(sr + 1);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_crack_lengths_fetch: out of host memory for %lld rows", static_cast<long long>(rows));
  }
  if (out_id) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_id, cm.cl_ids.p + sf, sr * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_rows7)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rows7, cm.cl_table.p + cl::kRowWords * sf, cl::kRowWords * sr * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out_offsets) PCP_HIP_TRY(ctx, hipMemcpyAsync(off.data(), cm.cl_offsets.p + sf, (sr + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < off.size(); ++k) out_offsets[k] = off[k];
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

int pcp_crack_paths_fetch(pcp_context *ctx, int64_t first_entry, int64_t max_entries, int32_t *out_index, int64_t *out_entries) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_entries) *out_entries = 0;
  const CrackMap &cm = *ctx->crack;
  int64_t entries = 0;
  const int rc = crack_window(ctx, "pcp_crack_paths_fetch", CrackMap::kLengths, first_entry, max_entries, cm.cl_entries, &entries);
  if (rc != PCP_OK || entries == 0) return rc;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (out_index)
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_index, cm.cl_path.p + first_entry, static_cast<size_t>(entries) * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (out_entries) *out_entries = entries;
  return PCP_OK;
}

int pcp_crack_lengths_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, const uint64_t *sum_q,
                           uint64_t *out_pos, int32_t *out_id, int64_t *out_rows7, int64_t *out_offsets, int32_t *out_path,
                           int64_t *out_cracks, int64_t *out_path_points) {
  if (out_cracks) *out_cracks = 0;
  if (out_path_points) *out_path_points = 0;
  if (!cf::min_views_ok(min_views) || !gn::radius_ok(radius)) {
    set_global_error("pcp_crack_lengths_host: min_views %d outside %d..%d or radius %g outside [0.005, 1]", min_views, cf::kMinViewsLo,
                     cf::kMinViewsHi, static_cast<double>(radius));
    return PCP_ERR_INVALID;
  }
  if (n < 0 || n > cf::kHostMaxPoints || (n > 0 && (!xyz || !views))) {
    set_global_error("pcp_crack_lengths_host: n outside 0..65536 or a missing array");
    return PCP_ERR_INVALID;
  }
  cl::HostResult res;
  try {
    cl::lengths_brute(n, xyz, views, sum_q, min_views, gn::threshold_of(radius), res);
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_crack_lengths_host: out of host memory for %lld points", static_cast<long long>(n));
    return PCP_ERR_NOMEM;
  }
  if (out_pos) std::copy(res.pos.begin(), res.pos.end(), out_pos);
  if (out_id) std::copy(res.ids.begin(), res.ids.end(), out_id);
  if (out_rows7) std::copy(res.rows.begin(), res.rows.end(), out_rows7);
  if (out_offsets) std::copy(res.offsets.begin(), res.offsets.end(), out_offsets);
  if (out_path) std::copy(res.path.begin(), res.path.end(), out_path);
  if (out_cracks) *out_cracks = static_cast<int64_t>(res.ids.size());
  if (out_path_points) *out_path_points = static_cast<int64_t>(res.path.size());
  return PCP_OK;
}

}  // extern "C"
