// pcp_cell_search.hpp -- the search the radius stages share ("The cell-wave search"): local colour smoothing
// (pcp_colour_smooth.hip), the normals (pcp_normals.hip) and the map comparison (pcp_compare.hip) all need "every record
// within r of every query, exact integer sums", and all three get it here.  The map registration (pcp_register.hip) and the
// coarse registration's descriptors (pcp_coarse.hip) are members too.  Internal: included by those five units only.
//
// The view's points are binned into the uniform grid of the radius searches (build_radius_grid, pcp_grid.hip) and copied
// into cell order as 16-B records (x, y, z, a word of the stage's).  A work item is up to kCellQ consecutive places of ONE
// cell, one wavefront-sized workgroup each, one query per lane; its candidates are the (2 reach + 1)^2 rows of neighbouring
// cells, each a contiguous run of records, staged through LDS in tiles of kCellTile records and read back as wave-wide
// broadcasts.  A cell of any size is walked tile by tile (an all-duplicate cloud is one cell).  What a stage does with a
// candidate is a functor of its own; the sums it keeps are integers, so the order of the walk never shows in a result.
#pragma once

#include <algorithm>

#include "pcp_internal.hpp"

namespace pcp {

constexpr int kCellBlock = 256;   // the 1-D helper kernels
constexpr int kCellQ = 64;        // queries per work item: one wavefront, one cell
constexpr int kCellTile = 512;    // candidate records per LDS tile (8 KiB: ~20 one-wave workgroups per CU hide the LDS latency)
constexpr int kCellMaxRows = 25;  // (2 reach + 1)^2 rows of neighbouring cells, reach <= 2

static inline uint32_t cell_blocks(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kCellBlock))); }

// ---- device side ------------------------------------------------------------------------------------------------------------
// Records in cell order and, in the same pass, the flags of the places that open a work item.  The stage's functor gives
//   uint32_t word(int64_t k, int32_t v) const   the record's fourth word for place k, view index v = order[k]
//   bool opens(uint32_t word) const             whether a place with that word may open a work item
// Place k opens one when it may and is a multiple of kCellQ places after its cell's first place.
template <class Stage>
__global__ __launch_bounds__(kCellBlock) void k_cell_records(const float *__restrict__ gx, const float *__restrict__ gy,
                                                             const float *__restrict__ gz, const int32_t *__restrict__ order,
                                                             int64_t m, GridDesc g, const int32_t *__restrict__ start, Stage stage,
                                                             uint4 *__restrict__ rec, uint8_t *__restrict__ flag) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x;
  if (k >= m) return;
  const float x = gx[k], y = gy[k], z = gz[k];
  const uint32_t w = stage.word(k, order[k]);
  rec[k] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), w);
  int32_t ix, iy, iz;
  grid_coords(g, x, y, z, ix, iy, iz);
  const int64_t first = cell_start(g, start, iz, iy, ix);
  flag[k] = (stage.opens(w) && ((k - first) % kCellQ) == 0) ? 1 : 0;
}

// one opened work item: the places k0 .. k0 + n - 1 of cell (ix, iy, iz), n <= kCellQ, and the lane's query record (lane < n:
// place k0 + lane; the other lanes hold place k0's and do not count)
struct CellItem {
  int32_t k0, ix, iy, iz, n;
  uint4 q;
};

__device__ __forceinline__ CellItem cell_open(const uint4 *__restrict__ rec, const int32_t *__restrict__ items, const GridDesc &g,
                                              const int32_t *__restrict__ start) {
  CellItem it;
  it.k0 = items[blockIdx.x];
  const int lane = threadIdx.x;
  {
    const uint4 r0 = rec[it.k0];
    grid_coords(g, __uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), it.ix, it.iy, it.iz);
  }
  it.n = min(kCellQ, cell_start(g, start, it.iz, it.iy, it.ix + 1) - it.k0);
  it.q = rec[it.k0 + (lane < it.n ? lane : 0)];
  return it;
}

// Every record of the cells within reach of the item's cell, handed to visit(const uint4 &) on the lanes that are `visiting`.
// Every lane of the workgroup must call it (it holds barriers); rows are clipped at the box's faces.
template <class Visit>
__device__ __forceinline__ void cell_walk(const uint4 *__restrict__ rec, const GridDesc &g, const int32_t *__restrict__ start,
                                          const CellItem &it, bool visiting, Visit visit) {
  __shared__ uint4 tile[kCellTile];
  __shared__ int32_t row_b[kCellMaxRows], row_e[kCellMaxRows];
  const int lane = threadIdx.x;
  const int32_t R = g.reach, side = 2 * R + 1, rows = side * side;
  if (lane < rows) {
    const int32_t zz = it.iz + lane / side - R, yy = it.iy + lane % side - R;
    int32_t b = 0, e = 0;
    if (zz >= 0 && zz < g.nz && yy >= 0 && yy < g.ny) {
      b = cell_start(g, start, zz, yy, max(it.ix - R, 0));
      e = cell_start(g, start, zz, yy, min(it.ix + R, g.nx - 1) + 1);
    }
    row_b[lane] = b;
    row_e[lane] = e;
  }
  __syncthreads();  // the rows are there for every lane
  for (int32_t row = 0; row < rows; ++row) {
    const int32_t b = row_b[row], e = row_e[row];
    for (int32_t t0 = b; t0 < e; t0 += kCellTile) {
      const int32_t cnt = min(kCellTile, e - t0);
      __syncthreads();  // the previous tile has been read by every lane
      for (int32_t u = lane; u < cnt; u += kCellQ) tile[u] = rec[t0 + u];
      __syncthreads();  // the tile is there for every lane
      if (visiting) {
#pragma unroll 4
        for (int32_t u = 0; u < cnt; ++u) {
          const uint4 c = tile[u];
          visit(c);
        }
      }
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// per-call scratch of cell_search_prepare and what it hands back: owned by the caller, released when its call returns (a
// 10 M-point map holds ~200 MB of it)
struct CellSearch {
  GridDesc g;
  DevBuf<uint4> rec;       // the view's points in cell order
  DevBuf<int32_t> items;   // first place of every work item, ascending
  int64_t n_items = 0;
};

// The cv.n > 0 points of view cv made ready for the search kernel: the grid, the records, the work items.  `who` names the
// stage in messages, `slot` is the PCP_K_* slot the records launch is charged to, `flag` the caller's byte per place (grown
// here), item_capacity the most items the stage's functor can open.  compact_flags leaves its total in ctx->s_counter: a
// stage that tallies there clears it after this call.
template <class Stage>
int cell_search_prepare(pcp_context *ctx, const CloudView &cv, float radius, const char *who, int32_t slot, Stage stage,
                        int64_t item_capacity, DevBuf<uint8_t> &flag, CellSearch &cs) {
  const int64_t m = cv.n;
  int rc = build_radius_grid(ctx, cv, radius, &cs.g);
  if (rc != PCP_OK) return rc;
  // build_radius_grid's cell edge is at least 1.001 r, so reach = ceil(r / cell) is 1 in every call made today: the 25 rows
  // and "1..2" are the kernel's capacity, not a case that occurs.  The walk still reads reach at run time.
  if (cs.g.reach < 1 || (2 * cs.g.reach + 1) * (2 * cs.g.reach + 1) > kCellMaxRows)
    return set_error(ctx, PCP_ERR_INVALID, "%s: grid reach %d outside 1..2", who, cs.g.reach);
  const size_t gplane = (static_cast<size_t>(m) + 3) & ~size_t(3);
  PCP_HIP_TRY(ctx, cs.rec.ensure(static_cast<size_t>(m) + 4));
  PCP_HIP_TRY(ctx, flag.ensure(static_cast<size_t>(m) + 16));
  PCP_HIP_TRY(ctx, cs.items.ensure(static_cast<size_t>(item_capacity) + 4));
  {
    LaunchTimer lt(ctx, slot);
    hipLaunchKernelGGL(k_cell_records<Stage>, dim3(cell_blocks(m)), dim3(kCellBlock), 0, ctx->stream, ctx->g_xyz.p,
                       ctx->g_xyz.p + gplane, ctx->g_xyz.p + 2 * gplane, ctx->g_order.p, m, cs.g, ctx->g_start.p, stage, cs.rec.p,
                       flag.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  return compact_flags(ctx, flag.p, m, cs.items.p, item_capacity, &cs.n_items);
}

}  // namespace pcp
