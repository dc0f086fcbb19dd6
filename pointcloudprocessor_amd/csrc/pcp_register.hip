// pcp_register.hip -- map registration on gfx950 ("Map registration", RG1-RG9): the base survey of the map
// comparison is brought onto the uploaded map by point-to-plane ICP before pcp_compare measures the change.  The rule is
// pcp_register.hpp's: per sampled base row the nearest map point, thirty exact integer terms per pair, a fixed fp64 solve on
// the host.
// Search: the cell-wave search of pcp_cell_search.hpp over ONE grid (cell >= match_radius) for both clouds, here the base's
// current rows FIRST and the map's finite points after them, so that a cell's base records come before its map records and a
// work item is up to 64 BASE records of one cell, opened on base records only, by the shared rule as it is.  During the walk
// a lane minimises one 64-bit key; after it the lanes with a pair form their thirty terms, which are summed over the wavefront
// and added into one of kRgSlots partial slots; a small kernel folds the slots.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "pcp_cell_search.hpp"
#include "pcp_device.hpp"
#include "pcp_internal.hpp"
#include "pcp_normals.hpp"
#include "pcp_compare.hpp"
#include "pcp_register.hpp"

namespace pcp {

constexpr uint32_t kRgEpochBit = 0x80000000u;
constexpr int64_t kRgMaxPoints = (int64_t(1) << 31) - 64;  // RG5: n + n_base
constexpr int kRgSlots = 1024;                             // partial sums: slot = work item modulo kRgSlots
constexpr size_t kRgWords = kRgSlots * rg::kSumWords + rg::kSumWords + 8;  // the slots, the folded sums, a transform's box

// ---- RG1: the current rows from the original rows --------------------------------------------------------------------------
// a float as an unsigned word that orders as the float does (finite values)
__device__ __forceinline__ uint32_t rg_ordered(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static inline float rg_unordered(uint32_t w) {
  const uint32_t b = (w & 0x80000000u) ? (w & 0x7fffffffu) : ~w;
  float v;
  std::memcpy(&v, &b, 4);
  return v;
}

// rows k, k + gridDim.x * kCellBlock, .. per lane; box[0..2] = min, box[3..5] = max of the rows written, as ordered words.  The
// grid is capped (kRgTransformBlocks) and a workgroup folds its four wavefronts through LDS, so the six words take one atomic
// per workgroup: a few thousand in all, not one per wavefront of a 10 M-row base.
constexpr int kRgTransformBlocks = 2048;
__global__ __launch_bounds__(kCellBlock) void k_rg_transform(const float *__restrict__ x0, const float *__restrict__ y0,
                                                             const float *__restrict__ z0, int64_t m, rg::Frame f,
                                                             float *__restrict__ x1, float *__restrict__ y1, float *__restrict__ z1,
                                                             uint32_t *__restrict__ box) {
  __shared__ uint32_t part[kCellBlock / 64][6];
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  const int64_t step = static_cast<int64_t>(gridDim.x) * kCellBlock;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x; k < m; k += step) {
    float o[3];
    rg::apply(f, x0[k], y0[k], z0[k], o);
    x1[k] = o[0];
    y1[k] = o[1];
    z1[k] = o[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t w = rg_ordered(o[a]);
      lo[a] = min(lo[a], w);
      hi[a] = max(hi[a], w);
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_min_u32(lo[a]);
    hi[a] = wave_max_u32(hi[a]);
    if ((threadIdx.x & 63) == 0) {
      part[wave][a] = lo[a];
      part[wave][3 + a] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t v = part[0][threadIdx.x];
    for (int w = 1; w < kCellBlock / 64; ++w) v = threadIdx.x < 3 ? min(v, part[w][threadIdx.x]) : max(v, part[w][threadIdx.x]);
    // (a workgroup without a row leaves the neutral words: no effect)
    if (threadIdx.x < 3)
      atomicMin(box + threadIdx.x, v);
    else
      atomicMax(box + threadIdx.x, v);
  }
}

// the two clouds as one view, the BASE first: its mb current rows (tag = the caller's row with the epoch bit), then the map's
// ma finite points (tag = the caller's index)
__global__ __launch_bounds__(kCellBlock) void k_rg_concat(const float *__restrict__ bx, const float *__restrict__ by,
                                                          const float *__restrict__ bz, const uint32_t *__restrict__ btag, int64_t mb,
                                                          const float *__restrict__ ax, const float *__restrict__ ay,
                                                          const float *__restrict__ az, const int32_t *__restrict__ aremap, int64_t ma,
                                                          float *__restrict__ cx, float *__restrict__ cy, float *__restrict__ cz,
                                                          uint32_t *__restrict__ ctag) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x;
  if (k >= ma + mb) return;
  if (k < mb) {
    cx[k] = bx[k];
    cy[k] = by[k];
    cz[k] = bz[k];
    ctag[k] = btag[k];
  } else {
    const int64_t j = k - mb;
    cx[k] = ax[j];
    cy[k] = ay[j];
    cz[k] = az[j];
    ctag[k] = static_cast<uint32_t>(aremap ? aremap[j] : static_cast<int32_t>(j));
  }
}

// the record's word is the tag; only a base record opens a work item (a cell's base records come first)
struct RgStage {
  const uint32_t *tag;
  __device__ uint32_t word(int64_t, int32_t v) const { return tag[v]; }
  __device__ bool opens(uint32_t w) const { return (w & kRgEpochBit) != 0; }
};

// what k_rg_pairs needs beside the search
struct RgPairs {
  float t;
  int64_t tau2;
  uint32_t stride;
  double c[3];
  const float *mx, *my, *mz;  // the uploaded map, input order
  const float *normals;
  int32_t normal_stride;
};

// one work item: the base records k0 .. of one cell (up to kCellQ) against the map records of the neighbouring cells.
// slots: kRgSlots x rg::kSumWords words; the wavefront's sums go to slot blockIdx.x % kRgSlots, one atomic per word.
__global__ __launch_bounds__(kCellQ) void k_rg_pairs(const uint4 *__restrict__ rec, const int32_t *__restrict__ items, GridDesc g,
                                                     const int32_t *__restrict__ start, RgPairs a,
                                                     unsigned long long *__restrict__ slots) {
  const CellItem it = cell_open(rec, items, g, start);
  const int lane = threadIdx.x;
  const uint4 q = it.q;
  const uint32_t row = q.w & ~kRgEpochBit;
  // RG2 (the cell's map records follow its base records)
  const bool query = lane < it.n && (q.w & kRgEpochBit) && (row % a.stride) == 0;
  const float qx = __uint_as_float(q.x), qy = __uint_as_float(q.y), qz = __uint_as_float(q.z);
  uint64_t best = ~uint64_t(0);
  cell_walk(rec, g, start, it, query, [&](const uint4 &c) {
    // RG3: every operation rounded on its own (-ffp-contract=off); a base record never wins
    const uint64_t key = rg::key_of(__uint_as_float(c.x) - qx, __uint_as_float(c.y) - qy, __uint_as_float(c.z) - qz, c.w);
    const uint64_t k = (c.w & kRgEpochBit) ? ~uint64_t(0) : key;
    best = k < best ? k : best;
  });
  bool pair = query && rg::d2_of_key(best) <= a.t;  // (no candidate: the key's d2 is a NaN)
  rg::Pair pr{};
  if (pair) {
    const int64_t j = static_cast<int64_t>(best & 0xffffffffull);
    const float *nrm = a.normals + j * a.normal_stride;
    int32_t N[3];
    pair = rg::normal_of(nrm[0], nrm[1], nrm[2], N);
    if (pair) {
      const int64_t u[3] = {rg::lever_of(qx, a.c[0]), rg::lever_of(qy, a.c[1]), rg::lever_of(qz, a.c[2])};
      pair = rg::pair_of(a.tau2, a.mx[j] - qx, a.my[j] - qy, a.mz[j] - qz, N, u, pr);
    }
  }
  if (__ballot(pair) == 0) return;  // (wave-uniform)
  if (!pair) {
#pragma unroll
    for (int k = 0; k < 6; ++k) pr.g[k] = 0;
    pr.h = 0;
    pr.N2 = 0;
  }
  int64_t term[rg::kTerms];
  rg::terms_of(pr, term);
  term[rg::kTerms - 1] = pair ? 1 : 0;
  unsigned long long *slot = slots + static_cast<size_t>(blockIdx.x % kRgSlots) * rg::kSumWords;
#pragma unroll
  for (int k = 0; k < rg::kTerms; ++k) {
    const unsigned long long lo = wave_sum_u64(static_cast<unsigned long long>(rg::low_of(term[k])));
    const unsigned long long hi = wave_sum_u64(static_cast<unsigned long long>(rg::high_of(term[k])));
    if (lane == 0) {
      if (lo) atomicAdd(slot + 2 * k, lo);
      if (hi) atomicAdd(slot + 2 * k + 1, hi);
    }
  }
}

// one workgroup per word: the slots folded (integer adds: the order does not show)
__global__ __launch_bounds__(64) void k_rg_reduce(const unsigned long long *__restrict__ slots, unsigned long long *__restrict__ out) {
  const int w = blockIdx.x;
  unsigned long long s = 0;
  for (int k = threadIdx.x; k < kRgSlots; k += 64) s += slots[static_cast<size_t>(k) * rg::kSumWords + w];
  s = wave_sum_u64(s);
  if (threadIdx.x == 0) out[w] = s;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static void params_message(char *buf, size_t len, const char *who, const char *why, const pcp_register_params *p) {
  std::snprintf(buf, len, "%s: %s (match_radius %g, max_plane_distance %g, sample_stride %d, max_iterations %d, min_pairs %d, tolerance %g, cond_tol %g)",
                who, why, static_cast<double>(p->match_radius), static_cast<double>(p->max_plane_distance), p->sample_stride,
                p->max_iterations, p->min_pairs, p->tolerance, p->cond_tol);
}

static int rule_of(const pcp_context *ctx, const char *who, const pcp_register_params *p, rg::Rule *rule) {
  const char *why = rg::prepare(p->match_radius, p->max_plane_distance, p->sample_stride, p->max_iterations, p->min_pairs, p->tolerance,
                                p->cond_tol, rule);
  if (!why) return PCP_OK;
  char buf[512];
  params_message(buf, sizeof buf, who, why, p);
  if (ctx) return set_error(ctx, PCP_ERR_INVALID, "%s", buf);
  set_global_error("%s", buf);
  return PCP_ERR_INVALID;
}

// RG1: the first registration call after pcp_compare_set_base keeps the original rows and fixes the pivot
static int state_ready(pcp_context *ctx) {
  CompareState &cs = ctx->compare;
  RegisterState &rs = cs.reg;
  if (rs.live) return PCP_OK;
  const size_t pb = (static_cast<size_t>(cs.m_base) + 3) & ~size_t(3);
  PCP_HIP_TRY(ctx, rs.base0.ensure(3 * pb + 4));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(rs.base0.p, cs.base_xyz.p, (3 * pb + 4) * 4, hipMemcpyDeviceToDevice, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int a = 0; a < 3; ++a) rs.mn0[a] = cs.mn[a], rs.mx0[a] = cs.mx[a];
  rg::pivot_of(rs.mn0, rs.mx0, rs.c, &rs.ell);
  rg::set_identity(rs.T);
  rs.live = true;
  return PCP_OK;
}

// RG1: the rows pcp_compare sees, from the ORIGINAL rows and T; their box.  A compare result belonged to the old rows.
static int rows_update(pcp_context *ctx) {
  CompareState &cs = ctx->compare;
  RegisterState &rs = cs.reg;
  cs.result_live = false;
  const int64_t mb = cs.m_base;
  const size_t pb = (static_cast<size_t>(mb) + 3) & ~size_t(3);
  if (mb == 0) return PCP_OK;
  if (rg::is_identity(rs.T)) {
    PCP_HIP_TRY(ctx, hipMemcpyAsync(cs.base_xyz.p, rs.base0.p, (3 * pb + 4) * 4, hipMemcpyDeviceToDevice, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int a = 0; a < 3; ++a) cs.mn[a] = rs.mn0[a], cs.mx[a] = rs.mx0[a];
    return PCP_OK;
  }
  rg::Frame f;
  rg::rotation_of(rs.T.q, f.R);
  for (int a = 0; a < 3; ++a) f.c[a] = rs.c[a], f.t[a] = rs.T.t[a];
  PCP_HIP_TRY(ctx, rs.words.ensure(kRgWords));
  uint32_t *box = reinterpret_cast<uint32_t *>(rs.words.p + kRgSlots * rg::kSumWords + rg::kSumWords);  // (the last 8 words)
  uint32_t hbox[6];
  PCP_HIP_TRY(ctx, hipMemsetAsync(box, 0xff, 12, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(box + 3, 0, 12, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_rg_transform, dim3(std::min<uint32_t>(cell_blocks(mb), kRgTransformBlocks)), dim3(kCellBlock), 0, ctx->stream, rs.base0.p, rs.base0.p + pb,
                       rs.base0.p + 2 * pb, mb, f, cs.base_xyz.p, cs.base_xyz.p + pb, cs.base_xyz.p + 2 * pb, box);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  PCP_HIP_TRY(ctx, hipMemcpyAsync(hbox, box, sizeof hbox, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int a = 0; a < 3; ++a) cs.mn[a] = rg_unordered(hbox[a]), cs.mx[a] = rg_unordered(hbox[3 + a]);
  return PCP_OK;
}

// a transform whose rows could leave fp32 is refused before anything moves (the rows stay finite: the grid needs that)
static bool transform_in_reach(const RegisterState &rs, const rg::Transform &T) {
  for (int a = 0; a < 3; ++a)
    if (!(std::fabs(rs.c[a]) + std::fabs(T.t[a]) + 2.0 * rs.ell <= 1.0e37)) return false;
  return true;
}

// per-call scratch: released when the call returns
struct RgScratch {
  FiniteScratch fin;
  CloudView cv;
  DevBuf<float> cxyz, normals;
  DevBuf<uint32_t> ctag;
  DevBuf<uint8_t> flag;
  const float *d_normals = nullptr;
  int32_t normal_stride = 4;
};

// what every evaluation of a call shares: the map's finite view and the normals on the device
static int scratch_ready(pcp_context *ctx, const float *host_normals, RgScratch &s) {
  const size_t sn = static_cast<size_t>(ctx->n);
  s.d_normals = ctx->gn_normal.p;
  s.normal_stride = 4;
  if (host_normals) {
    PCP_HIP_TRY(ctx, s.normals.ensure(3 * sn + 4));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(s.normals.p, host_normals, 3 * sn * 4, hipMemcpyHostToDevice, ctx->stream));
    s.d_normals = s.normals.p;
    s.normal_stride = 3;
  }
  int rc = finite_view(ctx, /*with_remap=*/true, /*timing_slot=*/-1, s.fin, &s.cv);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, ctx->s_counter.ensure(8));
  return PCP_OK;
}

// RG2-RG5 at the current rows: the grid, the records, the work items, the search, the fold; sums on the host
static int evaluate(pcp_context *ctx, const rg::Rule &rule, RgScratch &s, int64_t sums[rg::kSumWords]) {
  CompareState &cs = ctx->compare;
  RegisterState &rs = cs.reg;
  for (int a = 0; a < rg::kSumWords; ++a) sums[a] = 0;
  const int64_t ma = s.cv.n, mb = cs.m_base, m = ma + mb;
  if (mb == 0) return PCP_OK;
  if (!rg::levers_hold(cs.mn, cs.mx, rs.c))
    return set_error(ctx, PCP_ERR_RANGE, "pcp_compare_register: the base reaches more than 1024 m from its box's midpoint (the lever arm's range)");
  if (ma == 0) return PCP_OK;
  const size_t pm = (static_cast<size_t>(m) + 3) & ~size_t(3), pb = (static_cast<size_t>(mb) + 3) & ~size_t(3);
  PCP_HIP_TRY(ctx, s.cxyz.ensure(3 * pm + 4));
  PCP_HIP_TRY(ctx, s.ctag.ensure(static_cast<size_t>(m) + 4));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_rg_concat, dim3(cell_blocks(m)), dim3(kCellBlock), 0, ctx->stream, cs.base_xyz.p, cs.base_xyz.p + pb,
                       cs.base_xyz.p + 2 * pb, cs.base_tag.p, mb, s.cv.x, s.cv.y, s.cv.z, s.cv.remap, ma, s.cxyz.p, s.cxyz.p + pm,
                       s.cxyz.p + 2 * pm, s.ctag.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  CloudView both{};
  both.x = s.cxyz.p;
  both.y = s.cxyz.p + pm;
  both.z = s.cxyz.p + 2 * pm;
  both.n = m;
  both.remap = nullptr;
  for (int a = 0; a < 3; ++a) {  // the union of the boxes
    both.mn[a] = std::min(s.cv.mn[a], cs.mn[a]);
    both.mx[a] = std::max(s.cv.mx[a], cs.mx[a]);
  }
  CellSearch search;
  int rc = cell_search_prepare(ctx, both, rule.match_radius, "pcp_compare_register", PCP_K_MISC, RgStage{s.ctag.p}, mb, s.flag, search);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, rs.words.ensure(kRgWords));
  unsigned long long *slots = rs.words.p, *out = rs.words.p + kRgSlots * rg::kSumWords;
  PCP_HIP_TRY(ctx, hipMemsetAsync(slots, 0, (kRgSlots * rg::kSumWords + rg::kSumWords) * 8, ctx->stream));
  const size_t plane = (static_cast<size_t>(ctx->n) + 3) & ~size_t(3);
  RgPairs a;
  a.t = rule.t;
  a.tau2 = rule.tau2;
  a.stride = static_cast<uint32_t>(rule.stride);
  for (int k = 0; k < 3; ++k) a.c[k] = rs.c[k];
  a.mx = ctx->xyz.p;
  a.my = ctx->xyz.p + plane;
  a.mz = ctx->xyz.p + 2 * plane;
  a.normals = s.d_normals;
  a.normal_stride = s.normal_stride;
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    if (search.n_items > 0)
      hipLaunchKernelGGL(k_rg_pairs, dim3(static_cast<uint32_t>(search.n_items)), dim3(kCellQ), 0, ctx->stream, search.rec.p,
                         search.items.p, search.g, ctx->g_start.p, a, slots);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_rg_reduce, dim3(rg::kSumWords), dim3(64), 0, ctx->stream, slots, out);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  PCP_HIP_TRY(ctx, hipMemcpyAsync(sums, out, rg::kSumWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (also: the search's scratch is released on return)
  drop_large_grid_bitmap(ctx);
  return PCP_OK;
}

// what the three context calls check alike
static int state_of(pcp_context *ctx, const char *who, const float *normals, bool need_cloud) {
  CompareState &cs = ctx->compare;
  if (need_cloud && !ctx->xyz.p) return set_error(ctx, PCP_ERR_STATE, "%s: no cloud uploaded", who);
  if (!cs.base_live) return set_error(ctx, PCP_ERR_STATE, "%s: no base (pcp_compare_set_base)", who);
  if (need_cloud && !normals && !ctx->gn_live)
    return set_error(ctx, PCP_ERR_STATE, "%s: no normals (pcp_estimate_normals on this cloud, or pass an array)", who);
  if (need_cloud && ctx->n + cs.n_base > kRgMaxPoints)
    return set_error(ctx, PCP_ERR_INVALID, "%s: %lld map points and %lld base rows are more than 2^31 - 64 together", who,
                     static_cast<long long>(ctx->n), static_cast<long long>(cs.n_base));
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  return state_ready(ctx);
}

hipError_t preload_register() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_rg_pairs));
}

}  // namespace pcp

using namespace pcp;

extern "C" {

void pcp_default_register_params(pcp_register_params *p) {
  if (!p) return;
  p->match_radius = 0.05f;
  p->max_plane_distance = 0.02f;
  p->sample_stride = 1;
  p->max_iterations = 20;
  p->min_pairs = 100;
  p->tolerance = 1e-5;
  p->cond_tol = rg::kDefaultCondTol;
}

int pcp_compare_register_sums(pcp_context *ctx, const pcp_register_params *p, const float *normals, int64_t *out_sums60) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!p || !out_sums60) return set_error(ctx, PCP_ERR_INVALID, "pcp_compare_register_sums: no parameters or no output");
  rg::Rule rule;
  int rc = rule_of(ctx, "pcp_compare_register_sums", p, &rule);
  if (rc != PCP_OK) return rc;
  if ((rc = state_of(ctx, "pcp_compare_register_sums", normals, true)) != PCP_OK) return rc;
  for (int a = 0; a < rg::kSumWords; ++a) out_sums60[a] = 0;
  if (ctx->n == 0) return PCP_OK;
  RgScratch s;
  if ((rc = scratch_ready(ctx, normals, s)) != PCP_OK) return rc;
  return evaluate(ctx, rule, s, out_sums60);
}

int pcp_register_solve_host(const int64_t *sums60, double ell, double cond_tol, double *out_update7, double *out_eigenvalues6,
                            int32_t *out_dof) {
  if (!sums60 || !(ell > 0.0) || !(ell <= 1.0e6) || !(cond_tol > 0.0) || !(cond_tol < 1.0)) {
    set_global_error("pcp_register_solve_host: no sums, ell %g outside (0, 1e6] or cond_tol %g outside (0, 1)", ell, cond_tol);
    return PCP_ERR_INVALID;
  }
  double update[6], eig[6];
  const int32_t dof = rg::solve(sums60, ell, cond_tol, update, eig);
  if (out_update7) {
    for (int a = 0; a < 6; ++a) out_update7[a] = update[a];
    out_update7[6] = rg::rms_of(sums60);
  }
  if (out_eigenvalues6)
    for (int a = 0; a < 6; ++a) out_eigenvalues6[a] = eig[a];
  if (out_dof) *out_dof = dof;
  return PCP_OK;
}

int pcp_compare_register(pcp_context *ctx, const pcp_register_params *p, const float *normals, double *out_T16, double *out_log,
                         int32_t *out_status) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!p) return set_error(ctx, PCP_ERR_INVALID, "pcp_compare_register: no parameters");
  rg::Rule rule;
  int rc = rule_of(ctx, "pcp_compare_register", p, &rule);
  if (rc != PCP_OK) return rc;
  if ((rc = state_of(ctx, "pcp_compare_register", normals, true)) != PCP_OK) return rc;
  RegisterState &rs = ctx->compare.reg;
  std::vector<double> log;
  try {
    log.assign(static_cast<size_t>(rule.max_iterations) * rg::kLogWords, 0.0);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_compare_register: out of host memory");
  }
  int32_t status[2] = {rg::kTooFewPairs, 0};
  int64_t sums[rg::kSumWords];
  if (ctx->n > 0) {
    RgScratch s;
    if ((rc = scratch_ready(ctx, normals, s)) != PCP_OK) return rc;
    const rg::Transform before = rs.T;
    rg::Transform T = rs.T;
    bool first = true;
    rc = rg::iterate(rule, rs.ell, T, [&](const rg::Transform &now, int64_t *out) {
      if (!first) {  // (the first evaluation is at the rows that are there)
        if (!transform_in_reach(rs, now)) return set_error(ctx, PCP_ERR_RANGE, "pcp_compare_register: the transform left the range of fp32 rows");
        rs.T = now;
        const int e = rows_update(ctx);
        if (e != PCP_OK) return e;
      }
      first = false;
      return evaluate(ctx, rule, s, out);
    }, sums, log.data(), status);
    ctx->compare.result_live = false;  // RG9: a result belonged to the rows before the call
    if (rc == PCP_OK && std::memcmp(&T, &rs.T, sizeof T) == 0) {
      // too few pairs: T is where the last evaluation found the rows, and they stay
    } else if (rc == PCP_OK && transform_in_reach(rs, T)) {
      rs.T = T;  // the last update was composed after the last evaluation: one more pass over the base brings the rows to it
      rc = rows_update(ctx);
    } else if (rc == PCP_OK) {
      rc = set_error(ctx, PCP_ERR_RANGE, "pcp_compare_register: the transform left the range of fp32 rows");
    }
    if (rc != PCP_OK) {  // an error leaves the base where it was
      rs.T = before;
      rows_update(ctx);
      return rc;
    }
  } else {
    log[0] = log[1] = 0.0;
    status[1] = 1;
  }
  if (out_T16) rg::matrix_of(rs.T, rs.c, out_T16);
  if (out_log) std::memcpy(out_log, log.data(), log.size() * sizeof(double));
  if (out_status) out_status[0] = status[0], out_status[1] = status[1];
  return PCP_OK;
}

int pcp_compare_base_transform(pcp_context *ctx, double *out_T16, double *out_pivot3, double *out_ell) {
  if (!ctx) return PCP_ERR_INVALID;
  const CompareState &cs = ctx->compare;
  if (!cs.base_live) return set_error(ctx, PCP_ERR_STATE, "pcp_compare_base_transform: no base (pcp_compare_set_base)");
  // a query makes no state: before the first registration call the transform is the identity about the pivot of the box
  // that pcp_compare_set_base left
  rg::Transform T;
  rg::set_identity(T);
  double c[3], ell;
  rg::pivot_of(cs.mn, cs.mx, c, &ell);
  if (cs.reg.live) {
    T = cs.reg.T;
    for (int a = 0; a < 3; ++a) c[a] = cs.reg.c[a];
    ell = cs.reg.ell;
  }
  if (out_T16) rg::matrix_of(T, c, out_T16);
  if (out_pivot3)
    for (int a = 0; a < 3; ++a) out_pivot3[a] = c[a];
  if (out_ell) *out_ell = ell;
  return PCP_OK;
}

int pcp_compare_set_base_transform(pcp_context *ctx, const double *T16) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!T16) return set_error(ctx, PCP_ERR_INVALID, "pcp_compare_set_base_transform: no matrix");
  if (!ctx->compare.base_live) return set_error(ctx, PCP_ERR_STATE, "pcp_compare_set_base_transform: no base (pcp_compare_set_base)");
  // (the matrix is judged before any state is made)
  {
    const double zero[3] = {0.0, 0.0, 0.0};
    rg::Transform probe;
    if (!rg::from_matrix(T16, zero, &probe))
      return set_error(ctx, PCP_ERR_INVALID, "pcp_compare_set_base_transform: not a rigid motion (last row 0 0 0 1, rotation orthonormal to 1e-9, det > 0)");
  }
  int rc = state_of(ctx, "pcp_compare_set_base_transform", nullptr, false);
  if (rc != PCP_OK) return rc;
  RegisterState &rs = ctx->compare.reg;
  rg::Transform T;
  rg::from_matrix(T16, rs.c, &T);
  if (!transform_in_reach(rs, T))
    return set_error(ctx, PCP_ERR_RANGE, "pcp_compare_set_base_transform: the transform would leave the range of fp32 rows");
  rs.T = T;
  return rows_update(ctx);
}

int pcp_compare_register_host(const pcp_register_params *p, int64_t n, const float *xyz, const float *normals, int64_t n_base,
                              const float *base_xyz, const double *T_in16, int32_t run_loop, int64_t *out_sums60, double *out_T16,
                              double *out_log, int32_t *out_status, float *out_rows) {
  if (!p) {
    set_global_error("pcp_compare_register_host: no parameters");
    return PCP_ERR_INVALID;
  }
  rg::Rule rule;
  int rc = rule_of(nullptr, "pcp_compare_register_host", p, &rule);
  if (rc != PCP_OK) return rc;
  if (n < 0 || n > 65536 || n_base < 0 || n_base > 65536 || (n > 0 && (!xyz || !normals)) || (n_base > 0 && !base_xyz)) {
    set_global_error("pcp_compare_register_host: n or n_base outside 0..65536 or a missing array");
    return PCP_ERR_INVALID;
  }
  // RG1: the box of the finite original rows, the pivot, the scale
  float mn0[3] = {0, 0, 0}, mx0[3] = {0, 0, 0};
  bool any = false;
  for (int64_t j = 0; j < n_base; ++j) {
    const float *r = base_xyz + 3 * j;
    if (!gn::finite3(r[0], r[1], r[2])) continue;
    for (int a = 0; a < 3; ++a) {
      mn0[a] = any ? std::min(mn0[a], r[a]) : r[a];
      mx0[a] = any ? std::max(mx0[a], r[a]) : r[a];
    }
    any = true;
  }
  double c[3], ell;
  rg::pivot_of(mn0, mx0, c, &ell);
  rg::Transform T;
  rg::set_identity(T);
  if (T_in16 && !rg::from_matrix(T_in16, c, &T)) {
    set_global_error("pcp_compare_register_host: T_in is not a rigid motion");
    return PCP_ERR_INVALID;
  }
  std::vector<float> rows;
  try {
    rows.assign(static_cast<size_t>(3 * n_base) + 4, 0.0f);
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_compare_register_host: out of host memory");
    return PCP_ERR_NOMEM;
  }
  float mn[3], mx[3];
  auto rows_update = [&](const rg::Transform &now) {
    rg::Frame f;
    rg::rotation_of(now.q, f.R);
    for (int a = 0; a < 3; ++a) f.c[a] = c[a], f.t[a] = now.t[a];
    const bool ident = rg::is_identity(now);
    bool first = true;
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0f;
    for (int64_t j = 0; j < n_base; ++j) {
      const float *r = base_xyz + 3 * j;
      float *o = rows.data() + 3 * j;
      if (!gn::finite3(r[0], r[1], r[2]) || ident) {
        o[0] = r[0], o[1] = r[1], o[2] = r[2];
      } else {
        rg::apply(f, r[0], r[1], r[2], o);
      }
      if (!gn::finite3(r[0], r[1], r[2])) continue;
      for (int a = 0; a < 3; ++a) {
        mn[a] = first ? o[a] : std::min(mn[a], o[a]);
        mx[a] = first ? o[a] : std::max(mx[a], o[a]);
      }
      first = false;
    }
  };
  int64_t violations = 0;
  auto evaluate_host = [&](const rg::Transform &now, int64_t *sums) -> int {
    rows_update(now);
    for (int a = 0; a < rg::kSumWords; ++a) sums[a] = 0;
    if (!any) return PCP_OK;
    if (!rg::levers_hold(mn, mx, c)) {
      set_global_error("pcp_compare_register_host: the base reaches more than 1024 m from its box's midpoint (the lever arm's range)");
      return PCP_ERR_RANGE;
    }
    const int64_t workers = std::max<int64_t>(1, std::min<int64_t>({8, static_cast<int64_t>(std::thread::hardware_concurrency()), n_base / 512}));
    std::vector<int64_t> part(static_cast<size_t>(workers) * (rg::kSumWords + 1), 0);
    auto span = [&](int64_t j0, int64_t j1, int64_t *acc) {
      for (int64_t j = j0; j < j1; ++j) {
        if (j % rule.stride != 0) continue;
        const float *b = rows.data() + 3 * j;
        if (!gn::finite3(base_xyz[3 * j], base_xyz[3 * j + 1], base_xyz[3 * j + 2])) continue;
        uint64_t best = ~uint64_t(0);
        for (int64_t i = 0; i < n; ++i) {
          const float *q = xyz + 3 * i;
          if (!gn::finite3(q[0], q[1], q[2])) continue;
          const uint64_t key = rg::key_of(q[0] - b[0], q[1] - b[1], q[2] - b[2], static_cast<uint32_t>(i));
          best = key < best ? key : best;
        }
        if (!(rg::d2_of_key(best) <= rule.t)) continue;
        const int64_t i = static_cast<int64_t>(best & 0xffffffffull);
        int32_t N[3];
        if (!rg::normal_of(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], N)) continue;
        const int64_t u[3] = {rg::lever_of(b[0], c[0]), rg::lever_of(b[1], c[1]), rg::lever_of(b[2], c[2])};
        const float dx = xyz[3 * i] - b[0], dy = xyz[3 * i + 1] - b[1], dz = xyz[3 * i + 2] - b[2];
        if (!rg::terms_hold(rule.tau2, dx, dy, dz, N, u)) acc[rg::kSumWords] += 1;  // RG4's ranges: asserted, never seen
        rg::Pair pr;
        if (!rg::pair_of(rule.tau2, dx, dy, dz, N, u, pr)) continue;
        int64_t term[rg::kTerms];
        rg::terms_of(pr, term);
        for (int k = 0; k < rg::kTerms; ++k) {
          acc[2 * k] += rg::low_of(term[k]);
          acc[2 * k + 1] += rg::high_of(term[k]);
        }
      }
    };
    std::vector<std::thread> pool;
    for (int64_t w = 1; w < workers; ++w)
      pool.emplace_back(span, n_base * w / workers, n_base * (w + 1) / workers, part.data() + w * (rg::kSumWords + 1));
    span(0, n_base / workers, part.data());
    for (std::thread &th : pool) th.join();
    for (int64_t w = 0; w < workers; ++w) {
      for (int a = 0; a < rg::kSumWords; ++a) sums[a] += part[static_cast<size_t>(w * (rg::kSumWords + 1) + a)];
      violations += part[static_cast<size_t>(w * (rg::kSumWords + 1) + rg::kSumWords)];
    }
    return PCP_OK;
  };
  int64_t sums[rg::kSumWords];
  std::vector<double> log(static_cast<size_t>(rule.max_iterations) * rg::kLogWords, 0.0);
  int32_t status[2] = {rg::kIterationLimit, 0};
  if (run_loop) {
    rc = rg::iterate(rule, ell, T, evaluate_host, sums, log.data(), status);
  } else {
    rc = evaluate_host(T, sums);
  }
  if (rc != PCP_OK) return rc;
  if (violations != 0) {
    set_global_error("pcp_compare_register_host: %lld pairs left the ranges of RG4 (a defect of the rule)", static_cast<long long>(violations));
    return PCP_ERR_RANGE;
  }
  rows_update(T);
  if (out_sums60) std::memcpy(out_sums60, sums, sizeof sums);
  if (out_T16) rg::matrix_of(T, c, out_T16);
  if (out_log && run_loop) std::memcpy(out_log, log.data(), log.size() * sizeof(double));
  if (out_status) out_status[0] = status[0], out_status[1] = status[1];
  if (out_rows) std::memcpy(out_rows, rows.data(), static_cast<size_t>(3 * n_base) * sizeof(float));
  return PCP_OK;
}

}  // extern "C"
