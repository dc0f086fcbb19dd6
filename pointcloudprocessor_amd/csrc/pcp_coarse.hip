// pcp_coarse.hip -- coarse registration on gfx950 ("Coarse registration", CG1-CG9): the base survey of the map
// comparison is brought near the uploaded map from an arbitrary pose, so that pcp_compare_register can finish.  The rule is
// pcp_coarse.hpp's.
// Descriptors: the cell-wave search of pcp_cell_search.hpp over ONE side's finite points, one query per lane; a lane that
// holds a keypoint bins every neighbour into its own column of a bin-major histogram in LDS (hist[bin][lane], 16 KiB beside
// the search's 8 KiB tile: a wavefront's 64 increments fall on 64 distinct words, no atomics, no scratch).
// Matching: one lane per query with its 64 values in 32 registers, the other side's descriptors staged through LDS in tiles of
// 64 and read back as wave-wide broadcasts; both directions are the same kernel with the sides swapped.
// Scoring: one workgroup per frame over the correspondences.  Hypotheses, consensus and the refit run on the host.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "pcp_cell_search.hpp"
#include "pcp_device.hpp"
#include "pcp_internal.hpp"
#include "pcp_normals.hpp"
#include "pcp_compare.hpp"
#include "pcp_register.hpp"
#include "pcp_coarse.hpp"

namespace pcp {

constexpr uint32_t kCgEpochBit = 0x80000000u;  // (the base's tags carry it: pcp_compare_set_base)
constexpr int kCgMatchTile = 64;               // candidate descriptors per LDS tile (8 KiB)
constexpr int kCgScoreBlock = 256;

// the record's word is the caller's row: the base's tag without its epoch bit, or the map's remap
struct CgStage {
  const uint32_t *tag;
  const int32_t *remap;
  __device__ uint32_t word(int64_t, int32_t v) const { return tag ? (tag[v] & ~kCgEpochBit) : static_cast<uint32_t>(remap ? remap[v] : v); }
  __device__ bool opens(uint32_t) const { return true; }
};

// view index -> caller's row of the base (the normals stage's remap)
__global__ __launch_bounds__(kCellBlock) void k_cg_rows(const uint32_t *__restrict__ tag, int64_t m, int32_t *__restrict__ rows) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCellBlock + threadIdx.x;
  if (k < m) rows[k] = static_cast<int32_t>(tag[k] & ~kCgEpochBit);
}

// what k_cg_descriptors needs beside the search
struct CgDescribe {
  float t;
  int64_t edge2[cg::kBins];
  uint32_t stride;
  int32_t min_neighbours, min_offplane_permille;
  const float *normals;
  int32_t normal_stride;
  uint32_t *desc;   // 32 words (64 x uint16) per slot
  uint32_t *total;
  uint8_t *state;
  float *xyz;
};

// one work item: the records k0 .. of one cell (up to kCellQ) against the records of the neighbouring cells; only the lanes
// that hold a keypoint visit
__global__ __launch_bounds__(kCellQ) void k_cg_descriptors(const uint4 *__restrict__ rec, const int32_t *__restrict__ items, GridDesc g,
                                                           const int32_t *__restrict__ start, CgDescribe a) {
  __shared__ uint32_t hist[cg::kDescWords * kCellQ];
  const CellItem it = cell_open(rec, items, g, start);
  const int lane = threadIdx.x;
  const uint4 q = it.q;
  const uint32_t row = q.w;
  bool key = lane < it.n && (row % a.stride) == 0;  // CG1
  int32_t N[3] = {0, 0, 0};
  if (key) {
    const float *nrm = a.normals + static_cast<int64_t>(row) * a.normal_stride;
    key = rg::normal_of(nrm[0], nrm[1], nrm[2], N);
  }
  if (__ballot(key) == 0) return;  // (wave-uniform, before the walk's barriers)
  cg::Axis ax;
  cg::axis_of(a.edge2, N, ax);
#pragma unroll 8
  for (int b = 0; b < cg::kDescWords; ++b) hist[b * kCellQ + lane] = 0;  // (a lane reads and writes its own column only)
  const float qx = __uint_as_float(q.x), qy = __uint_as_float(q.y), qz = __uint_as_float(q.z);
  cell_walk(rec, g, start, it, key, [&](const uint4 &c) {
    const int bin = cg::bin_of(ax, a.t, __uint_as_float(c.x) - qx, __uint_as_float(c.y) - qy, __uint_as_float(c.z) - qz);
    if (bin >= 0) hist[bin * kCellQ + lane] += 1;
  });
  if (!key) return;
  uint32_t n = 0, plane = 0;
  for (int b = 0; b < cg::kDescWords; ++b) {
    const uint32_t c = hist[b * kCellQ + lane];
    n += c;
    plane += (b % cg::kBins) == 0 ? c : 0u;
  }
  const int64_t slot = row / a.stride;
  const bool valid = cg::descriptor_ok(a.min_neighbours, a.min_offplane_permille, n, plane);
  uint32_t *out = a.desc + slot * (cg::kDescWords / 2);
  for (int b = 0; b < cg::kDescWords; b += 2) {
    const uint32_t lo = valid ? cg::scaled(hist[b * kCellQ + lane], n) : 0u, hi = valid ? cg::scaled(hist[(b + 1) * kCellQ + lane], n) : 0u;
    out[b / 2] = lo | (hi << 16);
  }
  a.total[slot] = n;
  a.state[slot] = valid ? 2 : 1;
  a.xyz[3 * slot + 0] = qx;
  a.xyz[3 * slot + 1] = qy;
  a.xyz[3 * slot + 2] = qz;
}

// CG3: query ordinal k (slot slot_q[k] of desc_q) against the m candidates (slots slot_c of desc_c); out: best, second
__global__ __launch_bounds__(kCellQ) void k_cg_match(const uint32_t *__restrict__ desc_q, const int32_t *__restrict__ slot_q, int64_t kq,
                                                     const uint32_t *__restrict__ desc_c, const int32_t *__restrict__ slot_c, int64_t m,
                                                     unsigned long long *__restrict__ out) {
  constexpr int kW = cg::kDescWords / 2;
  __shared__ uint32_t tile[kCgMatchTile * kW];
  const int lane = threadIdx.x;
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kCellQ + lane;
  const bool active = k < kq;
  uint32_t mine[kW];
  {
    const uint32_t *src = desc_q + static_cast<int64_t>(slot_q[active ? k : 0]) * kW;
#pragma unroll
    for (int w = 0; w < kW; ++w) mine[w] = src[w];
  }
  cg::Best best{cg::kNoKey, cg::kNoKey};
  for (int64_t m0 = 0; m0 < m; m0 += kCgMatchTile) {
    const int cnt = static_cast<int>(min(static_cast<int64_t>(kCgMatchTile), m - m0));
    __syncthreads();  // the previous tile has been read by every lane
    for (int u = lane; u < cnt * kW; u += kCellQ) tile[u] = desc_c[static_cast<int64_t>(slot_c[m0 + u / kW]) * kW + u % kW];
    __syncthreads();  // the tile is there for every lane
    if (active) {
      for (int c = 0; c < cnt; ++c) {
        uint32_t l1 = 0;
#pragma unroll
        for (int w = 0; w < kW; ++w) {
          const uint32_t x = tile[c * kW + w], y = mine[w];
          const int32_t d0 = static_cast<int32_t>(x & 0xffffu) - static_cast<int32_t>(y & 0xffffu);
          const int32_t d1 = static_cast<int32_t>(x >> 16) - static_cast<int32_t>(y >> 16);
          l1 += static_cast<uint32_t>(d0 < 0 ? -d0 : d0) + static_cast<uint32_t>(d1 < 0 ? -d1 : d1);
        }
        cg::offer(best, (static_cast<uint64_t>(l1) << 32) | static_cast<uint64_t>(m0 + c));
      }
    }
  }
  if (active) {
    out[2 * k] = best.best;
    out[2 * k + 1] = best.second;
  }
}

// CG5: one workgroup per frame; counts[f] = its inliers; flags (nullable): one byte per frame and correspondence
__global__ __launch_bounds__(kCgScoreBlock) void k_cg_score(const rg::Frame *__restrict__ frames, const float *__restrict__ cb,
                                                            const float *__restrict__ cm, int64_t c, int64_t tau2,
                                                            unsigned long long *__restrict__ counts, uint8_t *__restrict__ flags) {
  __shared__ unsigned long long part[kCgScoreBlock / 64];
  const rg::Frame f = frames[blockIdx.x];
  unsigned long long mine = 0;
  for (int64_t k = threadIdx.x; k < c; k += kCgScoreBlock) {
    const bool in = cg::inlier_pair(f, tau2, cb + 3 * k, cm + 3 * k);
    mine += in ? 1 : 0;
    if (flags) flags[static_cast<int64_t>(blockIdx.x) * c + k] = in ? 1 : 0;
  }
  mine = wave_sum_u64(mine);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < kCgScoreBlock / 64; ++w) s += part[w];
    counts[blockIdx.x] = s;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int rule_of(const pcp_context *ctx, const char *who, const pcp_coarse_params *p, cg::Rule *rule) {
  const char *why = cg::prepare(*p, rule);
  if (!why) return PCP_OK;
  char buf[640];
  std::snprintf(buf, sizeof buf,
                "%s: %s (support_radius %g, normal_radius %g, inlier_distance %g, min_side %g, side_tolerance %g, min_angle_deg %g, strides %d %d, "
                "min_neighbours %d, min_offplane_permille %d, ratio_q8 %d, mutual %d, hypotheses %d, min_inliers %d)",
                who, why, static_cast<double>(p->support_radius), static_cast<double>(p->normal_radius), static_cast<double>(p->inlier_distance),
                static_cast<double>(p->min_side), static_cast<double>(p->side_tolerance), static_cast<double>(p->min_angle_deg), p->map_stride,
                p->base_stride, p->min_neighbours, p->min_offplane_permille, p->ratio_q8, p->mutual, p->hypotheses, p->min_inliers);
  if (ctx) return set_error(ctx, PCP_ERR_INVALID, "%s", buf);
  set_global_error("%s", buf);
  return PCP_ERR_INVALID;
}

// CG7: the register stage's refusals
static int state_of(pcp_context *ctx, const char *who, bool need_cloud, bool need_base) {
  if (need_cloud && !ctx->xyz.p) return set_error(ctx, PCP_ERR_STATE, "%s: no cloud uploaded", who);
  if (need_base && !ctx->compare.base_live) return set_error(ctx, PCP_ERR_STATE, "%s: no base (pcp_compare_set_base)", who);
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  return PCP_OK;
}

// the base's ORIGINAL rows as a view (CG7), its box and the pivot a transform of it turns about
static void base_view(const pcp_context *ctx, CloudView *cv, double pivot[3]) {
  const CompareState &cs = ctx->compare;
  const RegisterState &rs = cs.reg;
  const size_t pb = (static_cast<size_t>(cs.m_base) + 3) & ~size_t(3);
  const float *rows = rs.live ? rs.base0.p : cs.base_xyz.p;
  cv->x = rows, cv->y = rows + pb, cv->z = rows + 2 * pb;
  cv->n = cs.m_base;
  cv->remap = nullptr;
  for (int a = 0; a < 3; ++a) cv->mn[a] = rs.live ? rs.mn0[a] : cs.mn[a], cv->mx[a] = rs.live ? rs.mx0[a] : cs.mx[a];
  double ell;
  rg::pivot_of(cv->mn, cv->mx, pivot, &ell);
  if (rs.live)
    for (int a = 0; a < 3; ++a) pivot[a] = rs.c[a];
}

// CG1: the base's normals estimated at `radius` over its original rows (kept until the base is replaced)
static int base_normals_ready(pcp_context *ctx, float radius) {
  CompareState &cs = ctx->compare;
  CoarseState &co = cs.coarse;
  if (co.base_normals_live && co.base_normals_radius == radius) return PCP_OK;
  co.base_normals_live = false;
  const size_t sn = static_cast<size_t>(cs.n_base);
  PCP_HIP_TRY(ctx, co.base_normals.ensure(4 * sn + 4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(co.base_normals.p, 0, (4 * sn + 4) * 4, ctx->stream));
  if (cs.m_base > 0) {
    DevBuf<int32_t> rows, count;
    PCP_HIP_TRY(ctx, rows.ensure(static_cast<size_t>(cs.m_base) + 4));
    PCP_HIP_TRY(ctx, count.ensure(sn + 4));
    hipLaunchKernelGGL(k_cg_rows, dim3(cell_blocks(cs.m_base)), dim3(kCellBlock), 0, ctx->stream, cs.base_tag.p, cs.m_base, rows.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
    CloudView cv;
    double pivot[3];
    base_view(ctx, &cv, pivot);
    cv.remap = rows.p;
    int64_t most = 0;
    int rc = normals_of_view(ctx, cv, radius, "pcp_compare_register_coarse", co.base_normals.p, count.p, &most);
    if (rc != PCP_OK) return rc;
    if (most >= gn::kMaxNeighbours)
      return set_error(ctx, PCP_ERR_RANGE, "pcp_compare_register_coarse: a base row has %lld neighbours within %g (2^22 or more could overflow the moments)",
                       static_cast<long long>(most), static_cast<double>(radius));
  }
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  co.base_normals_live = true;
  co.base_normals_radius = radius;
  return PCP_OK;
}

// CG1 + CG2 for one side
static int describe_side(pcp_context *ctx, const char *who, const cg::Rule &rule, int32_t side, const float *host_normals) {
  CompareState &cs = ctx->compare;
  CoarseSide &sd = cs.coarse.side[side];
  cs.coarse.match_live = false;
  sd.live = false;
  const int64_t rows = side == 0 ? ctx->n : cs.n_base;
  const int32_t stride = side == 0 ? rule.map_stride : rule.base_stride;
  const int64_t slots = div_up(rows, static_cast<int64_t>(stride));
  if (slots > cg::kMaxKeypoints)
    return set_error(ctx, PCP_ERR_RANGE, "%s: %lld rows at stride %d are more than 2^18 keypoints on side %d (raise the stride)", who,
                     static_cast<long long>(rows), stride, side);
  const size_t ss = static_cast<size_t>(slots);
  PCP_HIP_TRY(ctx, sd.desc.ensure(ss * cg::kDescWords + 8));
  PCP_HIP_TRY(ctx, sd.total.ensure(ss + 4));
  PCP_HIP_TRY(ctx, sd.state.ensure(ss + 16));
  PCP_HIP_TRY(ctx, sd.xyz.ensure(3 * ss + 4));
  PCP_HIP_TRY(ctx, hipMemsetAsync(sd.desc.p, 0, (ss * cg::kDescWords + 8) * 2, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(sd.total.p, 0, (ss + 4) * 4, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(sd.state.p, 0, ss + 16, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(sd.xyz.p, 0, (3 * ss + 4) * 4, ctx->stream));
  // the side's normals on the device
  DevBuf<float> normals;
  CgDescribe a;
  a.normals = side == 0 ? ctx->gn_normal.p : cs.coarse.base_normals.p;
  a.normal_stride = 4;
  if (host_normals && rows > 0) {
    PCP_HIP_TRY(ctx, normals.ensure(3 * static_cast<size_t>(rows) + 4));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(normals.p, host_normals, 3 * static_cast<size_t>(rows) * 4, hipMemcpyHostToDevice, ctx->stream));
    a.normals = normals.p;
    a.normal_stride = 3;
  }
  FiniteScratch fin;
  DevBuf<uint8_t> flag;
  CloudView cv{};
  CgStage stage{nullptr, nullptr};
  if (side == 0) {
    if (rows > 0) {
      int rc = finite_view(ctx, /*with_remap=*/true, /*timing_slot=*/-1, fin, &cv);
      if (rc != PCP_OK) return rc;
      stage.remap = cv.remap;
    }
  } else {
    double pivot[3];
    base_view(ctx, &cv, pivot);
    stage.tag = cs.base_tag.p;
  }
  if (cv.n > 0) {
    CellSearch search;
    int rc = cell_search_prepare(ctx, cv, rule.support_radius, who, PCP_K_MISC, stage, cv.n, flag, search);
    if (rc != PCP_OK) return rc;
    a.t = rule.t;
    for (int k = 0; k < cg::kBins; ++k) a.edge2[k] = rule.edge2[k];
    a.stride = static_cast<uint32_t>(stride);
    a.min_neighbours = rule.min_neighbours;
    a.min_offplane_permille = rule.min_offplane_permille;
    a.desc = reinterpret_cast<uint32_t *>(sd.desc.p);
    a.total = sd.total.p;
    a.state = sd.state.p;
    a.xyz = sd.xyz.p;
    {
      LaunchTimer lt(ctx, PCP_K_MISC);
      if (search.n_items > 0)
        hipLaunchKernelGGL(k_cg_descriptors, dim3(static_cast<uint32_t>(search.n_items)), dim3(kCellQ), 0, ctx->stream, search.rec.p,
                           search.items.p, search.g, ctx->g_start.p, a);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (also: the search's scratch is released on return)
    drop_large_grid_bitmap(ctx);
  }
  // the host's lists: the valid slots in ascending order and their coordinates
  std::vector<uint8_t> state;
  std::vector<float> xyz;
  try {
    state.assign(ss + 1, 0);
    xyz.assign(3 * ss + 1, 0.0f);
    sd.valid_slot.clear();
    sd.valid_xyz.clear();
    if (slots > 0) {
      PCP_HIP_TRY(ctx, hipMemcpyAsync(state.data(), sd.state.p, ss, hipMemcpyDeviceToHost, ctx->stream));
      PCP_HIP_TRY(ctx, hipMemcpyAsync(xyz.data(), sd.xyz.p, 3 * ss * 4, hipMemcpyDeviceToHost, ctx->stream));
      PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    sd.keypoints = 0;
    for (int64_t s = 0; s < slots; ++s) {
      sd.keypoints += state[static_cast<size_t>(s)] != 0 ? 1 : 0;
      if (state[static_cast<size_t>(s)] != 2) continue;
      sd.valid_slot.push_back(static_cast<int32_t>(s));
      for (int k = 0; k < 3; ++k) sd.valid_xyz.push_back(xyz[static_cast<size_t>(3 * s + k)]);
    }
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "%s: out of host memory", who);
  }
  sd.slots = slots;
  sd.live = true;
  return PCP_OK;
}

// what a descriptor call of one side checks and readies before describe_side
static int describe_entry(pcp_context *ctx, const char *who, const cg::Rule &rule, int32_t side, const float *host_normals) {
  int rc = state_of(ctx, who, side == 0, side == 1);
  if (rc != PCP_OK) return rc;
  if (side == 0 && !host_normals && !ctx->gn_live)
    return set_error(ctx, PCP_ERR_STATE, "%s: no normals (pcp_estimate_normals on this cloud, or pass an array)", who);
  if (side == 1 && !host_normals && (rc = base_normals_ready(ctx, rule.normal_radius)) != PCP_OK) return rc;
  return describe_side(ctx, who, rule, side, host_normals);
}

// CG3 on the device: both directions, then the list on the host
static int match_sides(pcp_context *ctx, const char *who, const cg::Rule &rule) {
  CoarseState &co = ctx->compare.coarse;
  co.match_live = false;
  const CoarseSide &mp = co.side[0], &bs = co.side[1];
  const int64_t km = static_cast<int64_t>(mp.valid_slot.size()), kb = static_cast<int64_t>(bs.valid_slot.size());
  try {
    co.keys[0].assign(static_cast<size_t>(2 * km), cg::kNoKey);
    co.keys[1].assign(static_cast<size_t>(2 * kb), cg::kNoKey);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "%s: out of host memory", who);
  }
  if (km > 0 && kb > 0) {
    DevBuf<int32_t> slots;
    DevBuf<unsigned long long> keys;
    PCP_HIP_TRY(ctx, slots.ensure(static_cast<size_t>(km + kb) + 4));
    PCP_HIP_TRY(ctx, keys.ensure(static_cast<size_t>(2 * (km + kb)) + 4));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(slots.p, mp.valid_slot.data(), static_cast<size_t>(km) * 4, hipMemcpyHostToDevice, ctx->stream));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(slots.p + km, bs.valid_slot.data(), static_cast<size_t>(kb) * 4, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t *dm = reinterpret_cast<const uint32_t *>(mp.desc.p), *db = reinterpret_cast<const uint32_t *>(bs.desc.p);
    {
      LaunchTimer lt(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_cg_match, dim3(static_cast<uint32_t>(div_up(km, static_cast<int64_t>(kCellQ)))), dim3(kCellQ), 0, ctx->stream, dm,
                         slots.p, km, db, slots.p + km, kb, keys.p);
      hipLaunchKernelGGL(k_cg_match, dim3(static_cast<uint32_t>(div_up(kb, static_cast<int64_t>(kCellQ)))), dim3(kCellQ), 0, ctx->stream, db,
                         slots.p + km, kb, dm, slots.p, km, keys.p + 2 * km);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    PCP_HIP_TRY(ctx, hipMemcpyAsync(co.keys[0].data(), keys.p, static_cast<size_t>(2 * km) * 8, hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(co.keys[1].data(), keys.p + 2 * km, static_cast<size_t>(2 * kb) * 8, hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  try {
    cg::correspondences(rule, kb, reinterpret_cast<const cg::Best *>(co.keys[1].data()), reinterpret_cast<const cg::Best *>(co.keys[0].data()),
                        co.pairs);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "%s: out of host memory", who);
  }
  if (static_cast<int64_t>(co.pairs.size() / 2) > cg::kMaxCorrespondences)
    return set_error(ctx, PCP_ERR_RANGE, "%s: %lld correspondences are more than 2^18", who, static_cast<long long>(co.pairs.size() / 2));
  co.match_live = true;
  return PCP_OK;
}

// the live correspondences' coordinates, host and device (per-call scratch)
struct CgPairs {
  int64_t c = 0;
  std::vector<float> cb, cm;
  DevBuf<float> d_cb, d_cm;
  DevBuf<rg::Frame> frames;
  DevBuf<unsigned long long> counts;
  DevBuf<uint8_t> flags;
};

static int pairs_ready(pcp_context *ctx, const char *who, CgPairs &pr) {
  const CoarseState &co = ctx->compare.coarse;
  pr.c = static_cast<int64_t>(co.pairs.size() / 2);
  try {
    pr.cb.assign(static_cast<size_t>(3 * pr.c) + 1, 0.0f);
    pr.cm.assign(static_cast<size_t>(3 * pr.c) + 1, 0.0f);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "%s: out of host memory", who);
  }
  for (int64_t k = 0; k < pr.c; ++k)
    for (int a = 0; a < 3; ++a) {
      pr.cb[static_cast<size_t>(3 * k + a)] = co.side[1].valid_xyz[static_cast<size_t>(3 * co.pairs[static_cast<size_t>(2 * k)] + a)];
      pr.cm[static_cast<size_t>(3 * k + a)] = co.side[0].valid_xyz[static_cast<size_t>(3 * co.pairs[static_cast<size_t>(2 * k + 1)] + a)];
    }
  PCP_HIP_TRY(ctx, pr.d_cb.ensure(static_cast<size_t>(3 * pr.c) + 4));
  PCP_HIP_TRY(ctx, pr.d_cm.ensure(static_cast<size_t>(3 * pr.c) + 4));
  if (pr.c > 0) {
    PCP_HIP_TRY(ctx, hipMemcpyAsync(pr.d_cb.p, pr.cb.data(), static_cast<size_t>(3 * pr.c) * 4, hipMemcpyHostToDevice, ctx->stream));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(pr.d_cm.p, pr.cm.data(), static_cast<size_t>(3 * pr.c) * 4, hipMemcpyHostToDevice, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return PCP_OK;
}

// CG5 on the device: counts[f]; flags (nullable): n_frames x c bytes
static int score_frames(pcp_context *ctx, CgPairs &pr, int64_t tau2, const rg::Frame *frames, int64_t n_frames, int64_t *counts,
                        uint8_t *flags) {
  if (n_frames == 0) return PCP_OK;
  const size_t nf = static_cast<size_t>(n_frames), nflags = nf * static_cast<size_t>(pr.c);
  PCP_HIP_TRY(ctx, pr.frames.ensure(nf));
  PCP_HIP_TRY(ctx, pr.counts.ensure(nf + 4));
  if (flags) PCP_HIP_TRY(ctx, pr.flags.ensure(nflags + 16));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(pr.frames.p, frames, nf * sizeof(rg::Frame), hipMemcpyHostToDevice, ctx->stream));
  {
    LaunchTimer lt(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_cg_score, dim3(static_cast<uint32_t>(n_frames)), dim3(kCgScoreBlock), 0, ctx->stream, pr.frames.p, pr.d_cb.p, pr.d_cm.p,
                       pr.c, tau2, pr.counts.p, flags ? pr.flags.p : static_cast<uint8_t *>(nullptr));
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
  PCP_HIP_TRY(ctx, hipMemcpyAsync(counts, pr.counts.p, nf * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (flags && nflags > 0) PCP_HIP_TRY(ctx, hipMemcpyAsync(flags, pr.flags.p, nflags, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

// the box of the finite rows of an interleaved host array, and whether there is one
static bool box_of(int64_t n, const float *xyz, float mn[3], float mx[3]) {
  bool any = false;
  for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0f;
  for (int64_t j = 0; j < n; ++j) {
    const float *r = xyz + 3 * j;
    if (!gn::finite3(r[0], r[1], r[2])) continue;
    for (int a = 0; a < 3; ++a) {
      mn[a] = any ? std::min(mn[a], r[a]) : r[a];
      mx[a] = any ? std::max(mx[a], r[a]) : r[a];
    }
    any = true;
  }
  return any;
}

// CG1 + CG2 by brute force: every slot of one cloud; violations: pairs that left CG2's ranges
static void describe_host(const cg::Rule &rule, int32_t stride, int64_t n, const float *xyz, const float *normals, uint16_t *desc,
                          uint32_t *total, uint8_t *state, int64_t *violations) {
  const int64_t slots = div_up(n, static_cast<int64_t>(stride));
  std::vector<int64_t> bad(8, 0);
  auto span = [&](int64_t s0, int64_t s1, int64_t *viol) {
    for (int64_t s = s0; s < s1; ++s) {
      const int64_t i = s * stride;
      const float *q = xyz + 3 * i;
      uint16_t *out = desc + s * cg::kDescWords;
      for (int b = 0; b < cg::kDescWords; ++b) out[b] = 0;
      total[s] = 0;
      state[s] = 0;
      int32_t N[3];
      if (!gn::finite3(q[0], q[1], q[2]) || !rg::normal_of(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], N)) continue;
      cg::Axis ax;
      cg::axis_of(rule.edge2, N, ax);
      uint32_t hist[cg::kDescWords] = {0};
      for (int64_t j = 0; j < n; ++j) {
        const float *c = xyz + 3 * j;
        if (!gn::finite3(c[0], c[1], c[2])) continue;
        const float dx = c[0] - q[0], dy = c[1] - q[1], dz = c[2] - q[2];
        const int bin = cg::bin_of(ax, rule.t, dx, dy, dz);
        if (bin < 0) continue;
        if (!cg::bins_hold(ax, dx, dy, dz)) *viol += 1;
        hist[bin] += 1;
      }
      uint32_t cnt = 0, plane = 0;
      for (int b = 0; b < cg::kDescWords; ++b) cnt += hist[b], plane += (b % cg::kBins) == 0 ? hist[b] : 0u;
      const bool valid = cg::descriptor_ok(rule.min_neighbours, rule.min_offplane_permille, cnt, plane);
      for (int b = 0; b < cg::kDescWords && valid; ++b) out[b] = cg::scaled(hist[b], cnt);
      total[s] = cnt;
      state[s] = valid ? 2 : 1;
    }
  };
  const int64_t workers = std::max<int64_t>(1, std::min<int64_t>({8, static_cast<int64_t>(std::thread::hardware_concurrency()), slots / 64}));
  std::vector<std::thread> pool;
  pool.reserve(static_cast<size_t>(workers));  // (nothing below throws while a worker runs)
  int64_t started = 1;
  try {
    for (; started < workers; ++started)
      pool.emplace_back(span, slots * started / workers, slots * (started + 1) / workers, &bad[static_cast<size_t>(started)]);
  } catch (const std::system_error &) {  // (the host refused a thread: its span and the later ones run here)
  }
  span(0, slots / workers, &bad[0]);
  for (int64_t w = started; w < workers; ++w) span(slots * w / workers, slots * (w + 1) / workers, &bad[static_cast<size_t>(w)]);
  for (std::thread &th : pool) th.join();
  for (int64_t w = 0; w < workers; ++w) *violations += bad[static_cast<size_t>(w)];
}

// CG3 by brute force over kq queries and m candidates (descriptors packed by ordinal)
static void match_host(int64_t kq, const uint16_t *dq, int64_t m, const uint16_t *dc, cg::Best *out) {
  for (int64_t k = 0; k < kq; ++k) {
    cg::Best b{cg::kNoKey, cg::kNoKey};
    for (int64_t c = 0; c < m; ++c)
      cg::offer(b, (static_cast<uint64_t>(cg::l1_of(dq + k * cg::kDescWords, dc + c * cg::kDescWords)) << 32) | static_cast<uint64_t>(c));
    out[k] = b;
  }
}

static void score_host(int64_t tau2, const rg::Frame *frames, int64_t n_frames, int64_t c, const float *cb, const float *cm, int64_t *counts,
                       uint8_t *flags) {
  for (int64_t f = 0; f < n_frames; ++f) {
    counts[f] = 0;
    for (int64_t k = 0; k < c; ++k) {
      const bool in = cg::inlier_pair(frames[f], tau2, cb + 3 * k, cm + 3 * k);
      counts[f] += in ? 1 : 0;
      if (flags) flags[f * c + k] = in ? 1 : 0;
    }
  }
}

static void frame_from15(const double *w, rg::Frame &f) {
  for (int a = 0; a < 9; ++a) f.R[a] = w[a];
  for (int a = 0; a < 3; ++a) f.c[a] = w[9 + a], f.t[a] = w[12 + a];
}
static void frame_to15(const rg::Frame &f, double *w) {
  for (int a = 0; a < 9; ++a) w[a] = f.R[a];
  for (int a = 0; a < 3; ++a) w[9 + a] = f.c[a], w[12 + a] = f.t[a];
}

// a host-only entry point's body: no bad_alloc of its vectors crosses the C boundary
template <class Body>
static int host_guard(const char *who, Body &&body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    set_global_error("%s: out of host memory", who);
    return PCP_ERR_NOMEM;
  }
}

hipError_t preload_coarse() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_cg_descriptors));
}

}  // namespace pcp

using namespace pcp;

extern "C" {

void pcp_default_coarse_params(pcp_coarse_params *p) {
  if (!p) return;
  p->support_radius = 0.2f;
  p->normal_radius = 0.1f;
  p->inlier_distance = 0.05f;
  p->min_side = 0.3f;
  p->side_tolerance = 0.05f;
  p->min_angle_deg = 15.0f;
  p->map_stride = 4;
  p->base_stride = 4;
  p->min_neighbours = 20;
  p->min_offplane_permille = 100;
  p->ratio_q8 = 230;
  p->mutual = 1;
  p->hypotheses = 4096;
  p->min_inliers = 10;
  p->seed = 1;
}

int pcp_coarse_descriptors(pcp_context *ctx, const pcp_coarse_params *p, int32_t side, const float *normals, int64_t *out_counts3) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!p || (side != 0 && side != 1)) return set_error(ctx, PCP_ERR_INVALID, "pcp_coarse_descriptors: no parameters, or side %d neither 0 nor 1", side);
  cg::Rule rule;
  int rc = rule_of(ctx, "pcp_coarse_descriptors", p, &rule);
  if (rc != PCP_OK) return rc;
  if ((rc = describe_entry(ctx, "pcp_coarse_descriptors", rule, side, normals)) != PCP_OK) return rc;
  const CoarseSide &sd = ctx->compare.coarse.side[side];
  if (out_counts3) out_counts3[0] = sd.slots, out_counts3[1] = sd.keypoints, out_counts3[2] = static_cast<int64_t>(sd.valid_slot.size());
  return PCP_OK;
}

int pcp_coarse_descriptors_fetch(pcp_context *ctx, int32_t side, uint16_t *out_desc64, uint32_t *out_total, uint8_t *out_state,
                                 float *out_xyz) {
  if (!ctx) return PCP_ERR_INVALID;
  if (side != 0 && side != 1) return set_error(ctx, PCP_ERR_INVALID, "pcp_coarse_descriptors_fetch: side %d neither 0 nor 1", side);
  const CoarseSide &sd = ctx->compare.coarse.side[side];
  if (!sd.live) return set_error(ctx, PCP_ERR_STATE, "pcp_coarse_descriptors_fetch: no descriptors of side %d (pcp_coarse_descriptors)", side);
  if (sd.slots == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t ss = static_cast<size_t>(sd.slots);
  if (out_desc64) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_desc64, sd.desc.p, ss * cg::kDescWords * 2, hipMemcpyDeviceToHost, ctx->stream));
  if (out_total) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_total, sd.total.p, ss * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_state) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_state, sd.state.p, ss, hipMemcpyDeviceToHost, ctx->stream));
  if (out_xyz) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_xyz, sd.xyz.p, 3 * ss * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

int pcp_compare_base_normals_fetch(pcp_context *ctx, float *out_normals) {
  if (!ctx) return PCP_ERR_INVALID;
  const CompareState &cs = ctx->compare;
  if (!cs.base_live || !cs.coarse.base_normals_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_compare_base_normals_fetch: no estimate of the base's normals (a coarse call without base_normals)");
  if (cs.n_base == 0 || !out_normals) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<float> rows;
  try {
    rows.resize(4 * static_cast<size_t>(cs.n_base));
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_compare_base_normals_fetch: out of host memory");
  }
  PCP_HIP_TRY(ctx, hipMemcpyAsync(rows.data(), cs.coarse.base_normals.p, rows.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int64_t j = 0; j < cs.n_base; ++j)
    for (int a = 0; a < 3; ++a) out_normals[3 * j + a] = rows[static_cast<size_t>(4 * j + a)];
  return PCP_OK;
}

int pcp_coarse_match(pcp_context *ctx, const pcp_coarse_params *p, int64_t *out_count) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!p) return set_error(ctx, PCP_ERR_INVALID, "pcp_coarse_match: no parameters");
  cg::Rule rule;
  int rc = rule_of(ctx, "pcp_coarse_match", p, &rule);
  if (rc != PCP_OK) return rc;
  const CoarseState &co = ctx->compare.coarse;
  if (!co.side[0].live || !co.side[1].live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_coarse_match: no descriptors of the %s (pcp_coarse_descriptors)", co.side[0].live ? "base" : "map");
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if ((rc = match_sides(ctx, "pcp_coarse_match", rule)) != PCP_OK) return rc;
  if (out_count) *out_count = static_cast<int64_t>(co.pairs.size() / 2);
  return PCP_OK;
}

int pcp_coarse_match_fetch(pcp_context *ctx, int32_t *out_pairs, uint64_t *out_base_keys, uint64_t *out_map_keys) {
  if (!ctx) return PCP_ERR_INVALID;
  const CoarseState &co = ctx->compare.coarse;
  if (!co.match_live) return set_error(ctx, PCP_ERR_STATE, "pcp_coarse_match_fetch: no match (pcp_coarse_match)");
  if (out_pairs && !co.pairs.empty()) std::memcpy(out_pairs, co.pairs.data(), co.pairs.size() * 4);
  if (out_base_keys && !co.keys[1].empty()) std::memcpy(out_base_keys, co.keys[1].data(), co.keys[1].size() * 8);
  if (out_map_keys && !co.keys[0].empty()) std::memcpy(out_map_keys, co.keys[0].data(), co.keys[0].size() * 8);
  return PCP_OK;
}

int pcp_coarse_score(pcp_context *ctx, const pcp_coarse_params *p, int64_t n_frames, const double *frames15, int64_t *out_counts,
                     uint8_t *out_flags) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!p || n_frames < 0 || n_frames > cg::kMaxHypotheses || (n_frames > 0 && (!frames15 || !out_counts)))
    return set_error(ctx, PCP_ERR_INVALID, "pcp_coarse_score: no parameters, %lld frames outside 0..65536, or a missing array", static_cast<long long>(n_frames));
  cg::Rule rule;
  int rc = rule_of(ctx, "pcp_coarse_score", p, &rule);
  if (rc != PCP_OK) return rc;
  if (!ctx->compare.coarse.match_live) return set_error(ctx, PCP_ERR_STATE, "pcp_coarse_score: no match (pcp_coarse_match)");
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<rg::Frame> frames;
  try {
    frames.resize(static_cast<size_t>(n_frames));
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "pcp_coarse_score: out of host memory");
  }
  for (int64_t f = 0; f < n_frames; ++f) frame_from15(frames15 + 15 * f, frames[static_cast<size_t>(f)]);
  CgPairs pr;
  if ((rc = pairs_ready(ctx, "pcp_coarse_score", pr)) != PCP_OK) return rc;
  return score_frames(ctx, pr, rule.tau2, frames.data(), n_frames, out_counts, out_flags);
}

int pcp_compare_register_coarse(pcp_context *ctx, const pcp_coarse_params *p, const float *normals, const float *base_normals,
                                int64_t *out_report16, double *out_T16, uint8_t *out_inliers) {
  const char *who = "pcp_compare_register_coarse";
  if (!ctx) return PCP_ERR_INVALID;
  if (!p) return set_error(ctx, PCP_ERR_INVALID, "%s: no parameters", who);
  cg::Rule rule;
  int rc = rule_of(ctx, who, p, &rule);
  if (rc != PCP_OK) return rc;
  if ((rc = state_of(ctx, who, true, true)) != PCP_OK) return rc;
  if (!normals && !ctx->gn_live) return set_error(ctx, PCP_ERR_STATE, "%s: no normals (pcp_estimate_normals on this cloud, or pass an array)", who);
  if ((rc = describe_entry(ctx, who, rule, 0, normals)) != PCP_OK) return rc;
  if ((rc = describe_entry(ctx, who, rule, 1, base_normals)) != PCP_OK) return rc;
  if ((rc = match_sides(ctx, who, rule)) != PCP_OK) return rc;
  const CoarseState &co = ctx->compare.coarse;
  CgPairs pr;
  if ((rc = pairs_ready(ctx, who, pr)) != PCP_OK) return rc;
  int64_t report[cg::kReportWords] = {0};
  report[cg::kKeyMap] = co.side[0].keypoints, report[cg::kKeyBase] = co.side[1].keypoints;
  report[cg::kValidMap] = static_cast<int64_t>(co.side[0].valid_slot.size());
  report[cg::kValidBase] = static_cast<int64_t>(co.side[1].valid_slot.size());
  report[cg::kCorrespondences] = pr.c;
  CloudView bv;
  double pivot_b[3], pivot_m[3], ell;
  base_view(ctx, &bv, pivot_b);
  {
    const CloudView mv = uploaded_view(ctx, true);  // (the host box of the map's finite coordinates)
    rg::pivot_of(mv.mn, mv.mx, pivot_m, &ell);
  }
  rg::Frame found;
  std::vector<uint8_t> inliers;
  int dev = PCP_OK;
  try {
    rc = cg::consensus(rule, pr.c, pr.cb.data(), pr.cm.data(), pivot_b, pivot_m, [&](const rg::Frame *frames, int64_t nf, int64_t *counts, uint8_t *flags) {
      dev = score_frames(ctx, pr, rule.tau2, frames, nf, counts, flags);
      return dev == PCP_OK ? 0 : 1;
    }, report, &found, inliers);
  } catch (const std::bad_alloc &) {
    return set_error(ctx, PCP_ERR_NOMEM, "%s: out of host memory", who);
  }
  if (rc > 0) return dev;
  if (rc < 0) return set_error(ctx, PCP_ERR_RANGE, "%s: an inlier lies more than 1024 m from its cloud's midpoint (the refit's range)", who);
  if (report[cg::kStatus] == cg::kFound) {
    double M[16];
    cg::matrix_of_frame(found, M);
    if ((rc = pcp_compare_set_base_transform(ctx, M)) != PCP_OK) return rc;  // CG7
  }
  if (out_report16) std::memcpy(out_report16, report, sizeof report);
  if (out_T16 && (rc = pcp_compare_base_transform(ctx, out_T16, nullptr, nullptr)) != PCP_OK) return rc;
  if (out_inliers && pr.c > 0) std::memcpy(out_inliers, inliers.data(), static_cast<size_t>(pr.c));
  return PCP_OK;
}

// ---- host only ----------------------------------------------------------------------------------------------------------
static int host_rule(const char *who, const pcp_coarse_params *p, cg::Rule *rule) {
  if (!p) {
    set_global_error("%s: no parameters", who);
    return PCP_ERR_INVALID;
  }
  return rule_of(nullptr, who, p, rule);
}

int pcp_coarse_descriptors_host(const pcp_coarse_params *p, int32_t side, int64_t n, const float *xyz, const float *normals,
                                uint16_t *out_desc64, uint32_t *out_total, uint8_t *out_state, int64_t *out_counts3) {
  return host_guard("pcp_coarse_descriptors_host", [&]() -> int {
    cg::Rule rule;
    int rc = host_rule("pcp_coarse_descriptors_host", p, &rule);
    if (rc != PCP_OK) return rc;
    if ((side != 0 && side != 1) || n < 0 || n > 65536 || (n > 0 && (!xyz || !normals || !out_desc64 || !out_total || !out_state))) {
      set_global_error("pcp_coarse_descriptors_host: side neither 0 nor 1, n outside 0..65536 or a missing array");
      return PCP_ERR_INVALID;
    }
    const int32_t stride = side == 0 ? rule.map_stride : rule.base_stride;
    const int64_t slots = div_up(n, static_cast<int64_t>(stride));
    int64_t violations = 0;
    if (n > 0) describe_host(rule, stride, n, xyz, normals, out_desc64, out_total, out_state, &violations);
    if (violations != 0) {
      set_global_error("pcp_coarse_descriptors_host: %lld pairs left the ranges of CG2 (a defect of the rule)", static_cast<long long>(violations));
      return PCP_ERR_RANGE;
    }
    if (out_counts3) {
      out_counts3[0] = slots, out_counts3[1] = out_counts3[2] = 0;
      for (int64_t s = 0; s < slots; ++s) out_counts3[1] += out_state[s] != 0 ? 1 : 0, out_counts3[2] += out_state[s] == 2 ? 1 : 0;
    }
    return PCP_OK;
  });
}

int pcp_coarse_match_host(const pcp_coarse_params *p, int64_t k_base, const uint16_t *base_desc64, int64_t k_map,
                          const uint16_t *map_desc64, int32_t *out_pairs, int64_t *out_count, uint64_t *out_base_keys,
                          uint64_t *out_map_keys) {
  return host_guard("pcp_coarse_match_host", [&]() -> int {
    cg::Rule rule;
    int rc = host_rule("pcp_coarse_match_host", p, &rule);
    if (rc != PCP_OK) return rc;
    if (k_base < 0 || k_base > 65536 || k_map < 0 || k_map > 65536 || (k_base > 0 && !base_desc64) || (k_map > 0 && !map_desc64)) {
      set_global_error("pcp_coarse_match_host: a count outside 0..65536 or a missing array");
      return PCP_ERR_INVALID;
    }
    std::vector<cg::Best> bb(static_cast<size_t>(k_base) + 1), mb(static_cast<size_t>(k_map) + 1);
    match_host(k_base, base_desc64, k_map, map_desc64, bb.data());
    match_host(k_map, map_desc64, k_base, base_desc64, mb.data());
    std::vector<int32_t> pairs;
    cg::correspondences(rule, k_base, bb.data(), mb.data(), pairs);
    if (out_pairs && !pairs.empty()) std::memcpy(out_pairs, pairs.data(), pairs.size() * 4);
    if (out_count) *out_count = static_cast<int64_t>(pairs.size() / 2);
    if (out_base_keys && k_base > 0) std::memcpy(out_base_keys, bb.data(), static_cast<size_t>(k_base) * 16);
    if (out_map_keys && k_map > 0) std::memcpy(out_map_keys, mb.data(), static_cast<size_t>(k_map) * 16);
    return PCP_OK;
  });
}

int pcp_coarse_hypothesis_host(const pcp_coarse_params *p, int64_t c, const float *cb, const float *cm, const double *pivot3, int32_t h,
                               int32_t *out_code, int32_t *out_triple3, double *out_frame15) {
  cg::Rule rule;
  int rc = host_rule("pcp_coarse_hypothesis_host", p, &rule);
  if (rc != PCP_OK) return rc;
  if (c < 1 || c > cg::kMaxCorrespondences || !cb || !cm || !pivot3 || h < 0 || h >= cg::kMaxHypotheses) {
    set_global_error("pcp_coarse_hypothesis_host: c outside 1..2^18, h outside 0..65535 or a missing array");
    return PCP_ERR_INVALID;
  }
  cg::Hypothesis hy;
  cg::hypothesis(rule, c, cb, cm, pivot3, static_cast<uint32_t>(h), hy);
  if (out_code) *out_code = hy.code;
  if (out_triple3)
    for (int s = 0; s < 3; ++s) out_triple3[s] = hy.triple[s];
  if (out_frame15) frame_to15(hy.f, out_frame15);
  return PCP_OK;
}

int pcp_coarse_score_host(const pcp_coarse_params *p, int64_t n_frames, const double *frames15, int64_t c, const float *cb,
                          const float *cm, int64_t *out_counts, uint8_t *out_flags) {
  return host_guard("pcp_coarse_score_host", [&]() -> int {
    cg::Rule rule;
    int rc = host_rule("pcp_coarse_score_host", p, &rule);
    if (rc != PCP_OK) return rc;
    if (n_frames < 0 || n_frames > cg::kMaxHypotheses || c < 0 || c > cg::kMaxCorrespondences || (n_frames > 0 && (!frames15 || !out_counts)) ||
        (c > 0 && (!cb || !cm))) {
      set_global_error("pcp_coarse_score_host: a count out of range or a missing array");
      return PCP_ERR_INVALID;
    }
    std::vector<rg::Frame> frames(static_cast<size_t>(n_frames));
    for (int64_t f = 0; f < n_frames; ++f) frame_from15(frames15 + 15 * f, frames[static_cast<size_t>(f)]);
    score_host(rule.tau2, frames.data(), n_frames, c, cb, cm, out_counts, out_flags);
    return PCP_OK;
  });
}

int pcp_coarse_refit_host(int64_t c, const float *cb, const float *cm, const uint8_t *flags, const double *pivot_base3,
                          const double *pivot_map3, double *out_frame15) {
  return host_guard("pcp_coarse_refit_host", [&]() -> int {
    if (c < 0 || c > cg::kMaxCorrespondences || (c > 0 && (!cb || !cm || !flags)) || !pivot_base3 || !pivot_map3 || !out_frame15) {
      set_global_error("pcp_coarse_refit_host: c outside 0..2^18 or a missing array");
      return PCP_ERR_INVALID;
    }
    rg::Frame f;
    if (cg::refit(c, cb, cm, flags, pivot_base3, pivot_map3, f) != 0) {
      set_global_error("pcp_coarse_refit_host: an inlier lies more than 1024 m from its cloud's midpoint (the refit's range)");
      return PCP_ERR_RANGE;
    }
    frame_to15(f, out_frame15);
    return PCP_OK;
  });
}

int pcp_compare_register_coarse_host(const pcp_coarse_params *p, int64_t n, const float *xyz, const float *normals, int64_t n_base,
                                     const float *base_xyz, const float *base_normals, int64_t *out_report16, double *out_T16,
                                     uint8_t *out_inliers) {
  const char *who = "pcp_compare_register_coarse_host";
  return host_guard(who, [&]() -> int {
    cg::Rule rule;
    int rc = host_rule(who, p, &rule);
    if (rc != PCP_OK) return rc;
    if (n < 0 || n > 65536 || n_base < 0 || n_base > 65536 || (n > 0 && (!xyz || !normals)) || (n_base > 0 && (!base_xyz || !base_normals))) {
      set_global_error("%s: n or n_base outside 0..65536 or a missing array", who);
      return PCP_ERR_INVALID;
    }
    const int64_t rows[2] = {n, n_base};
    const int32_t stride[2] = {rule.map_stride, rule.base_stride};
    const float *pts[2] = {xyz, base_xyz}, *nrm[2] = {normals, base_normals};
    std::vector<uint16_t> packed[2];
    std::vector<float> kxyz[2];
    int64_t report[cg::kReportWords] = {0};
    int64_t violations = 0;
    for (int s = 0; s < 2; ++s) {
      const int64_t slots = div_up(rows[s], static_cast<int64_t>(stride[s]));
      std::vector<uint16_t> desc(static_cast<size_t>(slots) * cg::kDescWords + 1);
      std::vector<uint32_t> total(static_cast<size_t>(slots) + 1);
      std::vector<uint8_t> state(static_cast<size_t>(slots) + 1);
      if (rows[s] > 0) describe_host(rule, stride[s], rows[s], pts[s], nrm[s], desc.data(), total.data(), state.data(), &violations);
      for (int64_t k = 0; k < slots; ++k) {
        report[cg::kKeyMap + s] += state[static_cast<size_t>(k)] != 0 ? 1 : 0;
        if (state[static_cast<size_t>(k)] != 2) continue;
        report[cg::kValidMap + s] += 1;
        packed[s].insert(packed[s].end(), desc.begin() + k * cg::kDescWords, desc.begin() + (k + 1) * cg::kDescWords);
        for (int a = 0; a < 3; ++a) kxyz[s].push_back(pts[s][3 * k * stride[s] + a]);
      }
    }
    if (violations != 0) {
      set_global_error("%s: %lld pairs left the ranges of CG2 (a defect of the rule)", who, static_cast<long long>(violations));
      return PCP_ERR_RANGE;
    }
    const int64_t km = report[cg::kValidMap], kb = report[cg::kValidBase];
    std::vector<cg::Best> bb(static_cast<size_t>(kb) + 1), mb(static_cast<size_t>(km) + 1);
    match_host(kb, packed[1].data(), km, packed[0].data(), bb.data());
    match_host(km, packed[0].data(), kb, packed[1].data(), mb.data());
    std::vector<int32_t> pairs;
    cg::correspondences(rule, kb, bb.data(), mb.data(), pairs);
    const int64_t c = static_cast<int64_t>(pairs.size() / 2);
    report[cg::kCorrespondences] = c;
    std::vector<float> cb(static_cast<size_t>(3 * c) + 1), cm(static_cast<size_t>(3 * c) + 1);
    for (int64_t k = 0; k < c; ++k)
      for (int a = 0; a < 3; ++a) {
        cb[static_cast<size_t>(3 * k + a)] = kxyz[1][static_cast<size_t>(3 * pairs[static_cast<size_t>(2 * k)] + a)];
        cm[static_cast<size_t>(3 * k + a)] = kxyz[0][static_cast<size_t>(3 * pairs[static_cast<size_t>(2 * k + 1)] + a)];
      }
    float mn[3], mx[3];
    double pivot_b[3], pivot_m[3], ell;
    box_of(n_base, base_xyz, mn, mx);
    rg::pivot_of(mn, mx, pivot_b, &ell);
    box_of(n, xyz, mn, mx);
    rg::pivot_of(mn, mx, pivot_m, &ell);
    rg::Frame found;
    std::vector<uint8_t> inliers;
    rc = cg::consensus(rule, c, cb.data(), cm.data(), pivot_b, pivot_m, [&](const rg::Frame *frames, int64_t nf, int64_t *counts, uint8_t *flags) {
      score_host(rule.tau2, frames, nf, c, cb.data(), cm.data(), counts, flags);
      return 0;
    }, report, &found, inliers);
    if (rc != 0) {
      set_global_error("%s: an inlier lies more than 1024 m from its cloud's midpoint (the refit's range)", who);
      return PCP_ERR_RANGE;
    }
    rg::Transform T;
    rg::set_identity(T);
    if (report[cg::kStatus] == cg::kFound) {
      double M[16];
      cg::matrix_of_frame(found, M);
      if (!rg::from_matrix(M, pivot_b, &T)) {
        set_global_error("%s: the frame found is no rigid motion", who);
        return PCP_ERR_INVALID;
      }
    }
    if (out_report16) std::memcpy(out_report16, report, sizeof report);
    if (out_T16) rg::matrix_of(T, pivot_b, out_T16);
    if (out_inliers && c > 0) std::memcpy(out_inliers, inliers.data(), static_cast<size_t>(c));
    return PCP_OK;
  });
}

}  // extern "C"
