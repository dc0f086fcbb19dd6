// pcp_grid.hip -- the uniform grid of the radius searches and the front end the radius stages share.
//
// build_grid bins a cloud view into cells on the device: cell histogram -> exclusive scan -> scatter -> per-cell order
// fix-up (so results do not depend on atomic arrival order).  It serves the MLS / SOR stages (pcp_mls.hip) and, through the
// front end below, the stages that search a fixed radius around every point of the uploaded cloud: local colour smoothing,
// normals and map comparison, whose search is written once in pcp_cell_search.hpp (a wavefront per cell), and the neighbour
// table of PCP_MATCH_RADIUS (pcp_match.hip) and pcp_close_pairs, which walk the cells per lane.  The front end: the uploaded cloud as a view (uploaded_view), its finite points as a view where it has
// others (finite_view: the grid needs finite coordinates), the grid with a density-limited cell (build_radius_grid) and
// the rule that a huge sparse bitmap is not kept (drop_large_grid_bitmap).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>

#include "pcp_internal.hpp"
#include "pcp_scan.hpp"

namespace pcp {

constexpr int kMB = 256;

static inline uint32_t blocks_of(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kMB))); }

// cell id and arrival rank of every input point; histogram in `count`.  The views are spatially ordered (Morton copy of
// the upload, survivors of it), so a wavefront's 64 points fall into a handful of cells: the lanes of one cell share one
// atomic (ranks by lane, i.e. by index) instead of queueing 64 returning atomics on a few addresses (545 -> 60 us per
// 10 M points); after kAggRounds distinct cells the remaining lanes go alone (an unordered view would have 64 of them).
constexpr int kAggRounds = 8;
__global__ __launch_bounds__(kMB) void k_grid_count(const float *__restrict__ x, const float *__restrict__ y,
                                                    const float *__restrict__ z, int64_t n, GridDesc g,
                                                    int32_t *__restrict__ cell, int32_t *__restrict__ rank,
                                                    int32_t *__restrict__ count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kMB + threadIdx.x;
  int32_t c = -1;
  if (i < n) {
    int32_t ix, iy, iz;
    grid_coords(g, x[i], y[i], z[i], ix, iy, iz);
    c = (iz * g.ny + iy) * g.nx + ix;
    cell[i] = c;
  }
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  bool todo = c >= 0;
  int32_t r = 0;
  for (int round = 0; round < kAggRounds; ++round) {
    const unsigned long long open = __ballot(todo);
    if (!open) break;
    const int32_t c0 = __shfl(c, __ffsll(open) - 1, 64);
    const bool mine = todo && c == c0;
    const unsigned long long same = __ballot(mine);
    if (mine) {
      int32_t base = 0;
      if ((same & below) == 0) base = atomicAdd(count + c0, static_cast<int32_t>(__popcll(same)));  // lowest lane of the cell
      base = __builtin_amdgcn_readfirstlane(base);
      r = base + static_cast<int32_t>(__popcll(same & below));
      todo = false;
    }
  }
  if (todo) r = atomicAdd(count + c, 1);
  if (i < n) rank[i] = r;
}

// Sparse form, step 1: one bit per occupied cell
__global__ __launch_bounds__(kMB) void k_grid_mark(const float *__restrict__ x, const float *__restrict__ y,
                                                   const float *__restrict__ z, int64_t n, GridDesc g,
                                                   unsigned long long *__restrict__ occ) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kMB + threadIdx.x;
  if (i >= n) return;
  int32_t ix, iy, iz;
  grid_coords(g, x[i], y[i], z[i], ix, iy, iz);
  const int64_t c = (static_cast<int64_t>(iz) * g.ny + iy) * g.nx + ix;
  const unsigned long long bit = 1ull << (c & 63);
  if (!(occ[c >> 6] & bit)) atomicOr(occ + (c >> 6), bit);  // spatially ordered views: most bits are set already
}
// step 2: set bits per word (scanned in place into the running popcount)
__global__ __launch_bounds__(kMB) void k_grid_popc(const unsigned long long *__restrict__ occ, int64_t words,
                                                   int32_t *__restrict__ count) {
  const int64_t w = static_cast<int64_t>(blockIdx.x) * kMB + threadIdx.x;
  if (w < words) count[w] = static_cast<int32_t>(__popcll(occ[w]));
}
// step 3: as k_grid_count, with the cell's place among the occupied cells as its id
__global__ __launch_bounds__(kMB) void k_grid_count_sparse(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ z, int64_t n, GridDesc g,
                                                           int32_t *__restrict__ cell, int32_t *__restrict__ rank,
                                                           int32_t *__restrict__ count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kMB + threadIdx.x;
  int32_t c = -1;
  if (i < n) {
    int32_t ix, iy, iz;
    grid_coords(g, x[i], y[i], z[i], ix, iy, iz);
    c = cell_rank(g, (static_cast<int64_t>(iz) * g.ny + iy) * g.nx + ix);
    cell[i] = c;
  }
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  bool todo = c >= 0;
  int32_t r = 0;
  for (int round = 0; round < kAggRounds; ++round) {
    const unsigned long long open = __ballot(todo);
    if (!open) break;
    const int32_t c0 = __shfl(c, __ffsll(open) - 1, 64);
    const bool mine = todo && c == c0;
    const unsigned long long same = __ballot(mine);
    if (mine) {
      int32_t base = 0;
      if ((same & below) == 0) base = atomicAdd(count + c0, static_cast<int32_t>(__popcll(same)));
      base = __builtin_amdgcn_readfirstlane(base);
      r = base + static_cast<int32_t>(__popcll(same & below));
      todo = false;
    }
  }
  if (todo) r = atomicAdd(count + c, 1);
  if (i < n) rank[i] = r;
}

__global__ __launch_bounds__(kMB) void k_grid_scatter(int64_t n, const int32_t *__restrict__ cell,
                                                      const int32_t *__restrict__ rank,
                                                      const int32_t *__restrict__ start,
                                                      int32_t *__restrict__ order) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kMB + threadIdx.x;
  if (i >= n) return;
  order[start[cell[i]] + rank[i]] = static_cast<int32_t>(i);
}

// make the order inside every cell ascending in the input index (deterministic
// neighbour order), then gather the coordinates into cell order.  One lane per
// slot p of the scattered array: its point i = order_in[p] counts the members of
// its cell [b, e) that precede it.  The workgroup's 256 slots sit in LDS, and a
// cell holds a few dozen points, so nearly every comparison is an LDS read; the
// parts of a cell outside the window come from memory.  (The first version went
// through global memory for every member: 1.4 ms per 10 M-point SOR grid.)
__global__ __launch_bounds__(kMB) void k_grid_order(const float *__restrict__ x, const float *__restrict__ y,
                                                    const float *__restrict__ z, int64_t n, int64_t plane,
                                                    const int32_t *__restrict__ cell,
                                                    const int32_t *__restrict__ start,
                                                    const int32_t *__restrict__ order_in,
                                                    int32_t *__restrict__ order_out, float *__restrict__ sxyz) {
  __shared__ int32_t win[kMB];
  const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kMB;
  const int64_t p = w0 + threadIdx.x;
  const int32_t i = p < n ? order_in[p] : 0x7fffffff;
  win[threadIdx.x] = i;
  __syncthreads();
  if (p >= n) return;
  const int32_t c = cell[i];
  const int64_t b = start[c], e = start[c + 1];
  int32_t before = 0;
  const int64_t lb = max(b, w0), le = min(e, w0 + kMB);  // the part of the cell inside the window
  for (int64_t k = b; k < lb; ++k) before += order_in[k] < i ? 1 : 0;
  for (int64_t k = lb; k < le; ++k) before += win[k - w0] < i ? 1 : 0;
  for (int64_t k = max(le, b); k < e; ++k) before += order_in[k] < i ? 1 : 0;
  const int64_t j = b + before;
  order_out[j] = i;
  sxyz[j] = x[i];
  sxyz[plane + j] = y[i];
  sxyz[2 * plane + j] = z[i];
}

// uniform grid over a cloud view, cell edge >= `cell`; fills ctx->g_* (declared in pcp_internal.hpp)
int build_grid(pcp_context *ctx, const CloudView &cv, float cell, float radius, GridDesc *out, bool geometry_only) {
  const int64_t n = cv.n;
  GridDesc g{};
  const float *mn = cv.mn, *mx = cv.mx;
  for (int a = 0; a < 3; ++a)
    if (!(std::fabs(mn[a]) <= FLT_MAX) || !(std::fabs(mx[a]) <= FLT_MAX) || !(cell > 0.0f))
      return set_error(ctx, PCP_ERR_INVALID, "the smoothing stages need finite coordinates (bounding box %g .. %g on axis %d)",
                       static_cast<double>(mn[a]), static_cast<double>(mx[a]), a);
  // Up to kMaxGridCells cells the table of cell starts is dense (one int32 per cell, 2 GiB at most); up to
  // kMaxSparseCells it holds the occupied cells only, found through a bitmap with running popcounts (GridDesc; 6 GiB at
  // most).  A box that needs more cells than that at the wanted edge gets a coarser grid: the searches stay exact, every
  // doubling of the edge multiplies the candidates per query by up to 8 (a map with a stray point kilometres away).
  // PCP_GRID_SPARSE=1 / 0 forces the sparse / dense form (tests).
  const char *form_env = std::getenv("PCP_GRID_SPARSE");  // read per call: the tests flip it inside one process
  const int force_form = form_env ? (form_env[0] == '1' ? 1 : 0) : -1;
  const double cap = (force_form == 0 || geometry_only) ? kMaxGridCells : kMaxSparseCells;
  double cells = 0.0;
  for (int doubling = 0;; ++doubling) {  // bound the table: grow the cell until it fits
    const double ex = static_cast<double>(mx[0] - mn[0]) / cell + 1.0, ey = static_cast<double>(mx[1] - mn[1]) / cell + 1.0,
                 ez = static_cast<double>(mx[2] - mn[2]) / cell + 1.0;
    cells = ex * ey * ez;
    if (cells <= cap) break;
    if (doubling > 300) return set_error(ctx, PCP_ERR_INVALID, "no uniform grid fits this cloud's bounding box");
    cell *= 2.0f;
  }
  const bool sparse = !geometry_only && (force_form == 1 || cells > kMaxGridCells);
  g.minx = mn[0];
  g.miny = mn[1];
  g.minz = mn[2];
  g.inv_cell = 1.0f / cell;
  g.nx = static_cast<int32_t>(floorf((mx[0] - mn[0]) * g.inv_cell)) + 1;
  g.ny = static_cast<int32_t>(floorf((mx[1] - mn[1]) * g.inv_cell)) + 1;
  g.nz = static_cast<int32_t>(floorf((mx[2] - mn[2]) * g.inv_cell)) + 1;
  g.reach = static_cast<int32_t>(ceilf(radius * g.inv_cell));
  const int64_t ncell = static_cast<int64_t>(g.nx) * g.ny * g.nz;
  const size_t sn = static_cast<size_t>(n);
  const size_t plane = (sn + 3) & ~size_t(3);
  PCP_HIP_TRY(ctx, ctx->g_cell.ensure(sn + 4));
  PCP_HIP_TRY(ctx, ctx->g_rank.ensure(sn + 4));
  PCP_HIP_TRY(ctx, ctx->g_order.ensure(2 * sn + 8));
  {
    // k_sor_select<true> reads the planes in 16-byte pieces through one descriptor: a run's ragged end reads up to three
    // floats past the run -- the next cell's points, the up-to-3 floats of padding behind a plane, the start of the next plane
    // -- and masks those candidates by their x alone.  What it reads there must never be a NaN bit pattern (inf + NaN would
    // slip past the mask as NaN): the buffer only ever holds finite coordinates (non-finite clouds are refused) or, right
    // after an allocation, whatever hipMalloc left -- so a NEW allocation is zeroed once, and the padding stays non-NaN for
    // the buffer's life.
    const size_t before = ctx->g_xyz.count;  // (ensure() only ever grows: a changed count is a new allocation)
    PCP_HIP_TRY(ctx, ctx->g_xyz.ensure(3 * plane + 4));
    if (ctx->g_xyz.count != before) PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->g_xyz.p, 0, ctx->g_xyz.count * sizeof(float), ctx->stream));
  }
  if (geometry_only) {
    PCP_HIP_TRY(ctx, ctx->g_start.ensure(static_cast<size_t>(ncell) + 8));
    *out = g;
    return PCP_OK;
  }
  const float *x = cv.x, *y = cv.y, *z = cv.z;
  int64_t entries = ncell;  // entries of the table of cell starts (+ 1 for the total)
  if (sparse) {
    // occupied cells: one bit each; running popcount per word; the table gets one entry per set bit
    const int64_t words = ncell / 64 + 2;  // the lookups reach cell id ncell (one past the last)
    PCP_HIP_TRY(ctx, ctx->g_occ.ensure(static_cast<size_t>(words) + 2));
    PCP_HIP_TRY(ctx, ctx->g_occ_rank.ensure(static_cast<size_t>(words) + 8));
    PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->g_occ.p, 0, (static_cast<size_t>(words) + 2) * 8, ctx->stream));
    g.occ = ctx->g_occ.p;
    g.occ_rank = ctx->g_occ_rank.p;
    {
      LaunchTimer t(ctx, PCP_K_MLS_GRID);
      hipLaunchKernelGGL(k_grid_mark, dim3(blocks_of(n)), dim3(kMB), 0, ctx->stream, x, y, z, n, g, ctx->g_occ.p);
      hipLaunchKernelGGL(k_grid_popc, dim3(blocks_of(words)), dim3(kMB), 0, ctx->stream, ctx->g_occ.p, words, ctx->g_occ_rank.p);
      PCP_HIP_TRY(ctx, scan_exclusive(ctx->stream, ctx->g_occ_rank.p, words + 1, ctx->s_tiles, nullptr));  // [words] = the total
    }
    int32_t occupied = 0;
    PCP_HIP_TRY(ctx, hipMemcpyAsync(&occupied, ctx->g_occ_rank.p + words, 4, hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    entries = occupied;
  }
  PCP_HIP_TRY(ctx, ctx->g_start.ensure(static_cast<size_t>(entries) + 8));
  PCP_HIP_TRY(ctx, hipMemsetAsync(ctx->g_start.p, 0, (static_cast<size_t>(entries) + 8) * 4, ctx->stream));
  {
    LaunchTimer t(ctx, PCP_K_MLS_GRID);
    if (sparse)
      hipLaunchKernelGGL(k_grid_count_sparse, dim3(blocks_of(n)), dim3(kMB), 0, ctx->stream, x, y, z, n, g, ctx->g_cell.p,
                         ctx->g_rank.p, ctx->g_start.p);
    else
      hipLaunchKernelGGL(k_grid_count, dim3(blocks_of(n)), dim3(kMB), 0, ctx->stream, x, y, z, n, g, ctx->g_cell.p,
                         ctx->g_rank.p, ctx->g_start.p);
    PCP_HIP_TRY(ctx, scan_exclusive(ctx->stream, ctx->g_start.p, entries + 1, ctx->s_tiles, nullptr));  // [entries] = n
    hipLaunchKernelGGL(k_grid_scatter, dim3(blocks_of(n)), dim3(kMB), 0, ctx->stream, n, ctx->g_cell.p, ctx->g_rank.p,
                       ctx->g_start.p, ctx->g_order.p + sn + 4);
    hipLaunchKernelGGL(k_grid_order, dim3(blocks_of(n)), dim3(kMB), 0, ctx->stream, x, y, z, n,
                       static_cast<int64_t>(plane), ctx->g_cell.p, ctx->g_start.p, ctx->g_order.p + sn + 4,
                       ctx->g_order.p, ctx->g_xyz.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  *out = g;
  return PCP_OK;
}

// ---- the front end of the radius stages ------------------------------------------------------------------------------------
// 1 = point j of the Morton-ordered copy has three finite coordinates
__global__ __launch_bounds__(kMB) void k_grid_finite(const float *__restrict__ x, const float *__restrict__ y,
                                                     const float *__restrict__ z, int64_t n, uint8_t *__restrict__ flag) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kMB + threadIdx.x;
  if (j >= n) return;
  flag[j] = (fabsf(x[j]) <= FLT_MAX && fabsf(y[j]) <= FLT_MAX && fabsf(z[j]) <= FLT_MAX) ? 1 : 0;
}

// the finite points as a view: point k of the view = Morton point pos[k]; vremap[k] = its caller's index (nullable)
__global__ __launch_bounds__(kMB) void k_grid_gather(const float *__restrict__ x, const float *__restrict__ y,
                                                     const float *__restrict__ z, const int32_t *__restrict__ perm,
                                                     const int32_t *__restrict__ pos, int64_t m, float *__restrict__ vx,
                                                     float *__restrict__ vy, float *__restrict__ vz,
                                                     int32_t *__restrict__ vremap) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kMB + threadIdx.x;
  if (k >= m) return;
  const int32_t j = pos[k];
  vx[k] = x[j];
  vy[k] = y[j];
  vz[k] = z[j];
  if (vremap) vremap[k] = perm[j];
}

CloudView uploaded_view(const pcp_context *ctx, bool with_remap) {
  CloudView cv{};
  const size_t plane = (static_cast<size_t>(ctx->n) + 3) & ~size_t(3);
  cv.x = ctx->sxyz.p;
  cv.y = ctx->sxyz.p + plane;
  cv.z = ctx->sxyz.p + 2 * plane;
  cv.remap = with_remap ? ctx->perm.p : nullptr;
  cv.n = ctx->n;
  for (int a = 0; a < 3; ++a) {  // the box of the finite coordinates (a superset of the finite points' box)
    cv.mn[a] = ctx->host_min[static_cast<size_t>(a)];
    cv.mx[a] = ctx->host_max[static_cast<size_t>(a)];
  }
  return cv;
}

int finite_view(pcp_context *ctx, bool with_remap, int32_t timing_slot, FiniteScratch &s, CloudView *cv, const int32_t **pos) {
  *cv = uploaded_view(ctx, with_remap);
  if (pos) *pos = nullptr;
  if (ctx->nonfinite_points == 0) return PCP_OK;
  pcp_context *timed = timing_slot >= 0 ? ctx : nullptr;
  const int64_t n = ctx->n;
  const size_t sn = static_cast<size_t>(n);
  PCP_HIP_TRY(ctx, s.flag.ensure(sn + 16));
  PCP_HIP_TRY(ctx, s.pos.ensure(sn + 4));
  {
    LaunchTimer t(timed, timing_slot);
    hipLaunchKernelGGL(k_grid_finite, dim3(blocks_of(n)), dim3(kMB), 0, ctx->stream, cv->x, cv->y, cv->z, n, s.flag.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  int64_t m = 0;
  int rc = compact_flags(ctx, s.flag.p, n, s.pos.p, n, &m);
  if (rc != PCP_OK) return rc;
  const size_t pm = (static_cast<size_t>(m) + 3) & ~size_t(3);
  PCP_HIP_TRY(ctx, s.vxyz.ensure(3 * pm + 4));
  if (with_remap) PCP_HIP_TRY(ctx, s.vremap.ensure(static_cast<size_t>(m) + 4));
  if (m > 0) {
    LaunchTimer t(timed, timing_slot);
    hipLaunchKernelGGL(k_grid_gather, dim3(blocks_of(m)), dim3(kMB), 0, ctx->stream, cv->x, cv->y, cv->z, ctx->perm.p, s.pos.p, m,
                       s.vxyz.p, s.vxyz.p + pm, s.vxyz.p + 2 * pm, s.vremap.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  cv->x = s.vxyz.p;
  cv->y = s.vxyz.p + pm;
  cv->z = s.vxyz.p + 2 * pm;
  cv->remap = s.vremap.p;
  cv->n = m;
  if (pos) *pos = s.pos.p;
  return PCP_OK;
}

int build_radius_grid(pcp_context *ctx, const CloudView &cv, float radius, GridDesc *out) {
  // build_grid replaces the grid that an open MLS stream or a pcp_sor_partial rests on (as every call that builds one does)
  end_smoothing_streams(ctx);
  ctx->sor_partial_slab = ctx->sor_partial_slabs = -1;
  // Cell edge: the radius, but never finer than ~8 cells per point.  A micrometre radius on a map tens of metres across
  // would otherwise take the finest grid there is (2^35 cells: 6 GiB of bitmap and running popcounts, a 4 GiB memset
  // and a scan over 2^29 words, all for one count -- ADVICE r2); with the coarser cell the search is as exact (reach =
  // ceil(radius / cell) = 1, every pair closer than the radius lies in adjacent cells) and the table stays a few
  // entries per point.
  const double vol = std::max<double>(cv.mx[0] - cv.mn[0], 1e-3) * std::max<double>(cv.mx[1] - cv.mn[1], 1e-3) *
                     std::max<double>(cv.mx[2] - cv.mn[2], 1e-3);
  const float by_density = static_cast<float>(std::cbrt(vol / (8.0 * static_cast<double>(cv.n))));
  const float cell = std::max(radius * 1.001f, by_density);
  return build_grid(ctx, cv, cell, radius, out);
}

void drop_large_grid_bitmap(pcp_context *ctx) {
  if (ctx->g_occ.count > (size_t(1) << 25)) {
    ctx->g_occ.release();
    ctx->g_occ_rank.release();
  }
}

// (pcp_create loads every code object of the library up front: see preload_code_objects in pcp_context.hip)
hipError_t preload_grid() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_grid_order));
}

}  // namespace pcp
