// pcp_match.hip -- the neighbour table of PCP_MATCH_RADIUS, the reference's whole match-back
// (PointCloudProcessor.cpp:480-482,555,571-592): kdtree.radiusSearch(p_w, 1e-5) over the original cloud credits a sample
// to EVERY map point within 10 um of its fp32 world position p_w, not only to the point it came from.
//
// A sample of point i lies within E of p_i (E: a proven bound of the fp32 round-trip displacement |c2w(w2c p) - p|, below),
// so a point j can only receive it when |p_i - p_j| < r + E, r = 1e-5.  The table holds, for every point, the points within
// R_c = (r + E)(1 + 1e-3) of it (fp32 L2_Simple distance, strict <; the relation is symmetric because fl(a - b) = -fl(b - a)),
// itself included.  A = the points whose row holds more than that point.  Every credit to a point of A comes from a point of
// A, and a point outside A is credited by its own samples only: the colour pass serves it exactly as PCP_MATCH_ROUNDTRIP
// does, and k_match_fixup (pcp_colour.hip) recomputes, for each point of A, the samples of its row.
//
// Build (device): the finite points go into the uniform grid of the radius searches (pcp_grid.hip; cell >= R_c,
// reach 1); a count pass, an int64 exclusive scan over the rows of A, and a fill pass that also sorts each row by input index.
// The table is built at the first colour pass in this mode and lives until the cloud or the keyframes change.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "pcp_internal.hpp"

namespace pcp {

constexpr int kMtBlock = 256;

static inline uint32_t mt_blocks(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kMtBlock))); }

// fp32 L2_Simple as flann computes it: (dx^2 + dy^2) + dz^2, each operation rounded (no contraction: -ffp-contract=off)
__device__ __forceinline__ float mt_sqdist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  float d2 = dx * dx;
  d2 += dy * dy;
  d2 += dz * dz;
  return d2;
}

// count pass: per view point, the view points within R_c (itself included), stored at its Morton index
__global__ __launch_bounds__(kMtBlock) void k_mt_count(const float *__restrict__ vx, const float *__restrict__ vy,
                                                       const float *__restrict__ vz, const int32_t *__restrict__ vpos, int64_t m,
                                                       GridDesc g, const int32_t *__restrict__ start, const float *__restrict__ gx,
                                                       const float *__restrict__ gy, const float *__restrict__ gz, float rc2,
                                                       int32_t *__restrict__ count) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kMtBlock + threadIdx.x;
  if (v >= m) return;
  const float qx = vx[v], qy = vy[v], qz = vz[v];
  int32_t cx, cy, cz;
  grid_coords(g, qx, qy, qz, cx, cy, cz);
  int32_t c = 0;
  for (int32_t zz = max(cz - g.reach, 0); zz <= min(cz + g.reach, g.nz - 1); ++zz)
    for (int32_t yy = max(cy - g.reach, 0); yy <= min(cy + g.reach, g.ny - 1); ++yy) {
      const int32_t b = cell_start(g, start, zz, yy, max(cx - g.reach, 0));
      const int32_t e = cell_start(g, start, zz, yy, min(cx + g.reach, g.nx - 1) + 1);
      for (int32_t k = b; k < e; ++k) c += mt_sqdist(gx[k], gy[k], gz[k], qx, qy, qz) < rc2 ? 1 : 0;
    }
  count[vpos ? static_cast<int64_t>(vpos[v]) : v] = c;
}

__global__ __launch_bounds__(kMtBlock) void k_mt_flags(const int32_t *__restrict__ count, int64_t n, uint8_t *__restrict__ in_a) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kMtBlock + threadIdx.x;
  if (j < n) in_a[j] = count[j] > 1 ? 1 : 0;
}

__global__ __launch_bounds__(kMtBlock) void k_mt_row_len(const int32_t *__restrict__ count, const int32_t *__restrict__ list,
                                                         int64_t na, int64_t *__restrict__ len) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kMtBlock + threadIdx.x;
  if (k < na) len[k] = count[list[k]];
}

// ---- int64 exclusive scan (rows of A): block sums, one workgroup over the sums, per-block apply -------------------------
__device__ __forceinline__ long long mt_block_exclusive(long long v, long long *total, long long *ws /* [4] LDS */) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  long long incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) ws[wid] = incl;
  __syncthreads();
  long long base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kMtBlock / 64; ++k) {
    if (k < wid) base += ws[k];
    tot += ws[k];
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

__global__ __launch_bounds__(kMtBlock) void k_mt_scan_sums(const int64_t *__restrict__ v, int64_t m, int64_t *__restrict__ sums) {
  __shared__ long long ws[kMtBlock / 64];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kMtBlock + threadIdx.x;
  long long tot;
  (void)mt_block_exclusive(i < m ? v[i] : 0, &tot, ws);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// one workgroup: the block sums scanned in place, chunk by chunk with a carry; the grand total to *total
__global__ __launch_bounds__(kMtBlock) void k_mt_scan_top(int64_t *__restrict__ sums, int64_t nb, int64_t *__restrict__ total) {
  __shared__ long long ws[kMtBlock / 64];
  long long carry = 0;
  for (int64_t base = 0; base < nb; base += kMtBlock) {
    const int64_t i = base + threadIdx.x;
    long long tot;
    const long long ex = mt_block_exclusive(i < nb ? sums[i] : 0, &tot, ws);
    if (i < nb) sums[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kMtBlock) void k_mt_scan_apply(int64_t *__restrict__ v, int64_t m, const int64_t *__restrict__ sums) {
  __shared__ long long ws[kMtBlock / 64];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kMtBlock + threadIdx.x;
  long long tot;
  const long long ex = mt_block_exclusive(i < m ? v[i] : 0, &tot, ws);
  if (i < m) v[i] = sums[blockIdx.x] + ex;
}

// fill pass: the row of every point of A (Morton indices), then sorted by input index (insertion sort: rows are short, and a
// row of k entries costs k^2 here against k^2 x keyframes in the fix-up)
__global__ __launch_bounds__(kMtBlock) void k_mt_fill(const float *__restrict__ sx, const float *__restrict__ sy,
                                                      const float *__restrict__ sz, const int32_t *__restrict__ list, int64_t na,
                                                      const int64_t *__restrict__ off, GridDesc g, const int32_t *__restrict__ start,
                                                      const float *__restrict__ gx, const float *__restrict__ gy,
                                                      const float *__restrict__ gz, const int32_t *__restrict__ order,
                                                      const int32_t *__restrict__ vpos, const int32_t *__restrict__ perm,
                                                      float rc2, int32_t *__restrict__ cols) {
  const int64_t a = static_cast<int64_t>(blockIdx.x) * kMtBlock + threadIdx.x;
  if (a >= na) return;
  const int32_t j = list[a];
  const float qx = sx[j], qy = sy[j], qz = sz[j];
  const int64_t o = off[a], len = off[a + 1] - o;
  int32_t *row = cols + o;
  int32_t cx, cy, cz;
  grid_coords(g, qx, qy, qz, cx, cy, cz);
  int64_t c = 0;
  for (int32_t zz = max(cz - g.reach, 0); zz <= min(cz + g.reach, g.nz - 1); ++zz)
    for (int32_t yy = max(cy - g.reach, 0); yy <= min(cy + g.reach, g.ny - 1); ++yy) {
      const int32_t b = cell_start(g, start, zz, yy, max(cx - g.reach, 0));
      const int32_t e = cell_start(g, start, zz, yy, min(cx + g.reach, g.nx - 1) + 1);
      for (int32_t k = b; k < e; ++k)
        if (mt_sqdist(gx[k], gy[k], gz[k], qx, qy, qz) < rc2 && c < len) {
          const int32_t v = order[k];
          row[c++] = vpos ? vpos[v] : v;
        }
    }
  for (int64_t s = 1; s < c; ++s) {
    const int32_t t = row[s];
    const int32_t key = perm[t];
    int64_t b = s;
    while (b > 0 && perm[row[b - 1]] > key) {
      row[b] = row[b - 1];
      --b;
    }
    row[b] = t;
  }
}

// ---- E: a proven bound of |c2w(w2c p) - p| over the map's box -----------------------------------------------------------
// One row of xform (pcp_device.hpp): x c0 + (y c1 + (z c2 + c3)) in fp32.  With u = 2^-24 and every operation rounded to
// nearest, the six roundings are bounded by u times the magnitude of their exact results: the three products |x c0|, |y c1|,
// |z c2| and the partial sums, which are at most |z c2| + |c3|, |y c1| + |z c2| + |c3| and the full sum of magnitudes:
//   |err| <= u (2 |x c0| + 3 |y c1| + 4 |z c2| + 3 |c3|)   (second-order terms: the factor (1 + 8u) below).
static void row_bound(const float *m, const double q[3], double &mag, double &err) {
  const double a0 = std::fabs(static_cast<double>(m[0])) * q[0], a1 = std::fabs(static_cast<double>(m[1])) * q[1],
               a2 = std::fabs(static_cast<double>(m[2])) * q[2], a3 = std::fabs(static_cast<double>(m[3]));
  const double u = 0x1p-24;
  mag = a0 + a1 + a2 + a3;
  err = u * (1.0 + 8.0 * u) * (2.0 * a0 + 3.0 * a1 + 4.0 * a2 + 3.0 * a3);
}

// E over every keyframe of ctx.  For one keyframe with fp32 w2c = [A | a], c2w = [B | b] and |p_k| <= P_k:
//   p_c~ = A p + a + e1,                      |e1_r| <= row_bound(A_r, P)
//   p_w~ = B p_c~ + b + e2,                   |e2_r| <= row_bound(B_r, C), C_k = sum_m |A_km| P_m + |a_k| + |e1_k| >= |p_c~_k|
//   p_w~ - p = (BA - I) p + (Ba + b) + B e1 + e2
// so |d_r| <= sum_k |(BA - I)_rk| P_k + |(Ba + b)_r| + sum_k |B_rk| |e1_k| + |e2_r|, and E = max over keyframes of |d|.
// BA - I and Ba + b are formed in fp64 from the fp32 entries (products exact, sums of four terms within 4 ulp of fp64):
// the bound is padded by 1e-12 (relative to the terms) and 1e-6 relative, far above that rounding.
static double roundtrip_bound(const pcp_context *ctx) {
  double P[3];
  for (int a = 0; a < 3; ++a)
    P[a] = std::max(std::fabs(static_cast<double>(ctx->host_min[static_cast<size_t>(a)])),
                    std::fabs(static_cast<double>(ctx->host_max[static_cast<size_t>(a)])));
  double E = 0.0;
  for (const DevFrame &fr : ctx->hframes) {
    const float *A = fr.w2c, *B = fr.c2w;
    double e1[3], C[3];
    for (int r = 0; r < 3; ++r) {
      double mag, err;
      row_bound(A + 4 * r, P, mag, err);
      e1[r] = err;
      C[r] = mag + err;
    }
    double d2 = 0.0;
    for (int r = 0; r < 3; ++r) {
      double mag2, e2;
      row_bound(B + 4 * r, C, mag2, e2);
      double d = e2, scale = 0.0;
      for (int k = 0; k < 3; ++k) {
        double m = 0.0;
        for (int q = 0; q < 3; ++q) m += static_cast<double>(B[4 * r + q]) * static_cast<double>(A[4 * q + k]);
        if (r == k) m -= 1.0;
        d += std::fabs(m) * P[k] + std::fabs(static_cast<double>(B[4 * r + k])) * e1[k];
        scale += P[k] * 3.0;
      }
      double t = static_cast<double>(B[4 * r + 3]);
      for (int q = 0; q < 3; ++q) t += static_cast<double>(B[4 * r + q]) * static_cast<double>(A[4 * q + 3]);
      d += std::fabs(t);
      scale += std::fabs(static_cast<double>(B[4 * r + 3])) + 3.0 * C[r];
      d += 1e-12 * scale;
      d2 += d * d;
    }
    const double Ef = std::sqrt(d2) * (1.0 + 1e-6);
    if (!(Ef <= DBL_MAX)) return HUGE_VAL;
    E = std::max(E, Ef);
  }
  return E;
}

void match_table_release(pcp_context *ctx) {
  ctx->match_live = false;
  ctx->match_a = ctx->match_entries = 0;
  ctx->match_in_a.release();
  ctx->match_list.release();
  ctx->match_off.release();
  ctx->match_cols.release();
}

// per-build scratch, released on return
struct MtScratch {
  FiniteScratch fin;
  DevBuf<int32_t> count;
  DevBuf<int64_t> sums;
};

int match_table_prepare(pcp_context *ctx) {
  if (ctx->match_live) return PCP_OK;
  match_table_release(ctx);
  const int64_t n = ctx->n;
  const double r = static_cast<double>(1e-5f);  // radiusSearch(.., epsilon = 1e-5f), PointCloudProcessor.cpp:482
  const double E = roundtrip_bound(ctx);
  const double rc = (r + E) * (1.0 + 1e-3);
  // the table's relation is decided in fp32 (a few ulp of R_c^2): the 1e-3 margin covers that and the match test's own rounding
  if (!(rc <= 1e3))
    return set_error(ctx, PCP_ERR_INVALID, "PCP_MATCH_RADIUS: round-trip bound E = %g m (map or keyframe coordinates too large "
                     "or not finite)", E);
  ctx->match_e = E;
  ctx->match_rc = rc;
  {
    float e2 = static_cast<float>(E * E * (1.0 + 1e-6));
    if (static_cast<double>(e2) < E * E) e2 = std::nextafter(e2, FLT_MAX);
    ctx->match_e2 = e2;
  }
  const float rc2 = static_cast<float>(rc * rc);
  PCP_HIP_TRY(ctx, ctx->match_moved.ensure(4));
  const size_t sn = static_cast<size_t>(n);
  PCP_HIP_TRY(ctx, ctx->match_in_a.ensure(sn + 16));
  if (n == 0) {
    ctx->match_live = true;
    return PCP_OK;
  }
  MtScratch s;
  PCP_HIP_TRY(ctx, s.count.ensure(sn + 4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(s.count.p, 0, sn * 4, ctx->stream));  // non-finite points: count 0, not in A
  const size_t plane = (sn + 3) & ~size_t(3);
  CloudView cv;
  const int32_t *vpos;  // view index -> Morton index (nullptr: the same)
  // the grid needs finite coordinates; a non-finite point takes no sample and matches nothing
  int rcv = finite_view(ctx, /*with_remap=*/false, PCP_K_MISC, s.fin, &cv, &vpos);
  if (rcv != PCP_OK) return rcv;
  const int64_t m = cv.n;
  int64_t na = 0;
  GridDesc g{};
  if (m > 1) {
    int rcg = build_radius_grid(ctx, cv, static_cast<float>(rc), &g);
    if (rcg != PCP_OK) return rcg;
    const size_t gplane = (static_cast<size_t>(m) + 3) & ~size_t(3);
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_mt_count, dim3(mt_blocks(m)), dim3(kMtBlock), 0, ctx->stream, cv.x, cv.y, cv.z, vpos, m, g,
                         ctx->g_start.p, ctx->g_xyz.p, ctx->g_xyz.p + gplane, ctx->g_xyz.p + 2 * gplane, rc2, s.count.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
  }
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_mt_flags, dim3(mt_blocks(n)), dim3(kMtBlock), 0, ctx->stream, s.count.p, n, ctx->match_in_a.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  if (m > 1) {
    PCP_HIP_TRY(ctx, ctx->match_list.ensure(sn + 4));
    int rcc = compact_flags(ctx, ctx->match_in_a.p, n, ctx->match_list.p, n, &na);
    if (rcc != PCP_OK) return rcc;
  }
  if (na > 0) {
    PCP_HIP_TRY(ctx, ctx->match_off.ensure(static_cast<size_t>(na) + 4));
    const int64_t nb = div_up(na, kMtBlock);
    PCP_HIP_TRY(ctx, s.sums.ensure(static_cast<size_t>(nb) + 4));
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_mt_row_len, dim3(mt_blocks(na)), dim3(kMtBlock), 0, ctx->stream, s.count.p, ctx->match_list.p, na,
                         ctx->match_off.p);
      hipLaunchKernelGGL(k_mt_scan_sums, dim3(static_cast<uint32_t>(nb)), dim3(kMtBlock), 0, ctx->stream, ctx->match_off.p, na,
                         s.sums.p);
      hipLaunchKernelGGL(k_mt_scan_top, dim3(1), dim3(kMtBlock), 0, ctx->stream, s.sums.p, nb, ctx->match_off.p + na);
      hipLaunchKernelGGL(k_mt_scan_apply, dim3(static_cast<uint32_t>(nb)), dim3(kMtBlock), 0, ctx->stream, ctx->match_off.p, na,
                         s.sums.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    int64_t total = 0;
    PCP_HIP_TRY(ctx, hipMemcpyAsync(&total, ctx->match_off.p + na, 8, hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    PCP_HIP_TRY(ctx, ctx->match_cols.ensure(static_cast<size_t>(total) + 4));
    const size_t gplane = (static_cast<size_t>(m) + 3) & ~size_t(3);
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_mt_fill, dim3(mt_blocks(na)), dim3(kMtBlock), 0, ctx->stream, ctx->sxyz.p, ctx->sxyz.p + plane,
                         ctx->sxyz.p + 2 * plane, ctx->match_list.p, na, ctx->match_off.p, g, ctx->g_start.p, ctx->g_xyz.p,
                         ctx->g_xyz.p + gplane, ctx->g_xyz.p + 2 * gplane, ctx->g_order.p, vpos, ctx->perm.p, rc2,
                         ctx->match_cols.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    ctx->match_entries = total;
  } else {
    ctx->match_list.release();
  }
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the scratch is released on return)
  drop_large_grid_bitmap(ctx);  // (a large R_c on a sparse map may take the sparse grid)
  ctx->match_a = na;
  ctx->match_live = true;
  return PCP_OK;
}

// (pcp_create loads every code object of the library up front: see preload_code_objects in pcp_context.hip)
hipError_t preload_match() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_mt_fill));
}

}  // namespace pcp
