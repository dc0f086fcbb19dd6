// pcp_exposure.hip -- per-keyframe exposure gains from co-visible map points ("Exposure gains", EG1-EG5).  Two listed
// views of one point are two observations of the same surface element: the pair statistics over the top-5 state (EG3, exact
// integers), one gain per keyframe from a small least-squares problem on the host (EG4), and a finalise that applies the
// gains per listed view (EG5).  Opt-in: nothing here runs unless one of its entry points is called, and the plain finalise
// and the one-shot colour kernels keep their instruction streams.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <vector>

#include "pcp_internal.hpp"
#include "pcp_device.hpp"

namespace pcp {

constexpr int kExBlock = 256;
constexpr uint32_t kNoKey = 0xffffffffu;
constexpr int kExTableLog2 = 10;   // slots of the workgroup's table (16 KB of LDS); PCP_EXPOSURE_TABLE_LOG2 shrinks it (tests)
constexpr int kExProbes = 8;       // linear probes before a partial goes straight to global memory
constexpr int64_t kExMaxGrid = 2048;  // workgroups of the grid-stride pass: at most 2^20 points each for n < 2^31 (32-bit table sums)
constexpr int32_t kExMaxFrames = 4096;

// EG1: integer luma of a colour word 0x00RRGGBB (the caller masks the top byte)
__host__ __device__ __forceinline__ uint32_t luma_of(uint32_t c) {
  return (77u * ((c >> 16) & 0xffu) + 150u * ((c >> 8) & 0xffu) + 29u * (c & 0xffu) + 128u) >> 8;
}

// one unordered cell {lo, hi}, lo < hi, of the pair matrices: cnt pairs in either order, the lumas of the lo side and of the hi side
__device__ __forceinline__ void add_cell(unsigned long long *__restrict__ out_n, unsigned long long *__restrict__ out_sum, uint32_t F,
                                         uint32_t key, uint32_t cnt, uint32_t slo, uint32_t shi) {
  const uint32_t lo = key / F, hi = key - lo * F;
  const size_t a = static_cast<size_t>(lo) * F + hi, b = static_cast<size_t>(hi) * F + lo;
  atomicAdd(out_n + a, static_cast<unsigned long long>(cnt));
  atomicAdd(out_n + b, static_cast<unsigned long long>(cnt));
  atomicAdd(out_sum + a, static_cast<unsigned long long>(slo));
  atomicAdd(out_sum + b, static_cast<unsigned long long>(shi));
}

// EG3.  One lane per point of the state (its own order: the statistic does not depend on it), grid-stride over tiles of 256
// points.  The ordered pairs (a, b) and (b, a) of two slots share their condition, so the ten unordered slot pairs are walked
// with the key lo * F + hi, lo = min(f_a, f_b): cell (lo, hi) takes the count and the lo view's luma, cell (hi, lo) the count
// and the hi view's.  Neighbouring points list the same few keyframes, so a per-pair global add would serialise on a few
// cells.  Three levels instead:
//   wavefront: for every distinct key among the lanes (the first pending lane's key, a ballot of its equals) the count is a
//     popcount and the two luma sums are one cross-lane integer reduction of the packed pair -- exact;
//   workgroup: the leader adds the partial into an LDS table (open addressing, kExProbes linear probes, 32-bit sums: a
//     workgroup sees at most 2^20 points x 10 pairs x 247 < 2^32);
//   device: at the end every filled slot is flushed with four 64-bit adds.  A partial that finds no slot within its probes
//     (the table is full of other keys) is added to global memory directly.
// counters: [0] 64-bit adds issued at the flush, [1] adds issued directly (table full), [2] wavefront partials, [3] workgroups.
__global__ __launch_bounds__(kExBlock) void k_pair_stats(int64_t n, const uint32_t *__restrict__ rgb, const int32_t *__restrict__ frame,
                                                         uint32_t F, int32_t table_log2, unsigned long long *__restrict__ out_n,
                                                         unsigned long long *__restrict__ out_sum,
                                                         unsigned long long *__restrict__ counters) {
  extern __shared__ uint32_t ex_lds[];
  const uint32_t T = 1u << table_log2;
  uint32_t *keys = ex_lds, *t_cnt = ex_lds + T, *t_lo = ex_lds + 2 * T, *t_hi = ex_lds + 3 * T, *tally = ex_lds + 4 * T;
  for (uint32_t t = threadIdx.x; t < T; t += kExBlock) {
    keys[t] = kNoKey;
    t_cnt[t] = t_lo[t] = t_hi[t] = 0u;
  }
  if (threadIdx.x < 3) tally[threadIdx.x] = 0u;
  __syncthreads();
  const int lane = static_cast<int>(threadIdx.x & 63u);
  uint32_t direct = 0u, partials = 0u;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kExBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kExBlock) {
    const int64_t j = base + threadIdx.x;
    const bool live = j < n;
    int32_t v[kTopM];  // the slot's view, keyframe << 8 | luma; negative: empty, or not usable (EG2)
#pragma unroll
    for (int k = 0; k < kTopM; ++k) {
      const int32_t fk = live ? frame[k * n + j] : -1;
      const uint32_t c = live ? rgb[k * n + j] : 0u;
      const uint32_t yk = luma_of(c & 0xffffffu);  // (label fusion keeps the view's mask in the top byte)
      v[k] = (yk - 8u <= 239u && fk >= 0) ? static_cast<int32_t>((static_cast<uint32_t>(fk) << 8) | yk) : -1;
    }
#pragma unroll
    for (int a = 0; a < kTopM; ++a) {
#pragma unroll
      for (int b = a + 1; b < kTopM; ++b) {
        // ordered by keyframe without a select (equal keyframes are no pair, so the luma never decides the order)
        const int32_t vlo = min(v[a], v[b]), vhi = max(v[a], v[b]);
        const uint32_t lo = static_cast<uint32_t>(vlo) >> 8, hi = static_cast<uint32_t>(vhi) >> 8;
        const bool valid = vlo >= 0 && lo != hi;
        const uint32_t key = valid ? lo * F + hi : kNoKey;  // F <= 4096: below 2^24
        const uint32_t ylo = static_cast<uint32_t>(vlo) & 0xffu, yhi = static_cast<uint32_t>(vhi) & 0xffu;
        unsigned long long todo = __ballot(valid);
        while (todo) {  // uniform: todo is the same in every lane
          const int leader = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
          const uint32_t k0 = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(key), leader));
          const bool mine = key == k0;  // (k0 is a valid lane's key, never kNoKey)
          const unsigned long long same = __ballot(mine);
          const uint32_t cnt = static_cast<uint32_t>(__popcll(same));
          // both luma sums in one wavefront reduction: 64 lanes x 247 < 2^16 per half, no carry crosses
          const uint32_t both = __ockl_wfred_add_u32(mine ? ylo | (yhi << 16) : 0u);
          const uint32_t slo = both & 0xffffu, shi = both >> 16;
          if (lane == leader) {
            partials += 1u;
            const uint32_t h = table_log2 ? (k0 * 0x9e3779b1u) >> (32 - table_log2) : 0u;
            bool placed = false;
            for (int p = 0; p < kExProbes && !placed; ++p) {
              const uint32_t s = (h + static_cast<uint32_t>(p)) & (T - 1u);
              const uint32_t prev = atomicCAS(&keys[s], kNoKey, k0);
              if (prev == kNoKey || prev == k0) {
                atomicAdd(&t_cnt[s], cnt);
                atomicAdd(&t_lo[s], slo);
                atomicAdd(&t_hi[s], shi);
                placed = true;
              }
            }
            if (!placed) {
              add_cell(out_n, out_sum, F, k0, cnt, slo, shi);
              direct += 4u;
            }
          }
          todo &= ~same;
        }
      }
    }
  }
  __syncthreads();
  uint32_t flushed = 0u;
  for (uint32_t t = threadIdx.x; t < T; t += kExBlock) {
    const uint32_t k = keys[t];
    if (k != kNoKey) {
      add_cell(out_n, out_sum, F, k, t_cnt[t], t_lo[t], t_hi[t]);
      flushed += 4u;
    }
  }
  if (flushed) atomicAdd(&tally[0], flushed);
  if (direct) atomicAdd(&tally[1], direct);
  if (partials) atomicAdd(&tally[2], partials);
  __syncthreads();
  if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(counters + threadIdx.x, static_cast<unsigned long long>(tally[threadIdx.x]));
  if (threadIdx.x == 3) atomicAdd(counters + 3, 1ull);
}

// Top5::finalise over the gained channels (gained_channel: pcp_device.hpp); the label form also writes the label word, from the raw state (Top5::labels)
template <bool kLabel>
__global__ __launch_bounds__(kExBlock) void k_finalise_gained(int64_t n, const float *__restrict__ score, const uint32_t *__restrict__ rgb,
                                                              const int32_t *__restrict__ frame, const int32_t *__restrict__ count,
                                                              const int32_t *__restrict__ perm, const float *__restrict__ gains,
                                                              uint32_t *__restrict__ rgba, [[maybe_unused]] uint32_t *__restrict__ label_word) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kExBlock + threadIdx.x;
  if (j >= n) return;
  Top5 t;
  t.s0 = score[0 * n + j]; t.s1 = score[1 * n + j]; t.s2 = score[2 * n + j]; t.s3 = score[3 * n + j]; t.s4 = score[4 * n + j];
  t.c0 = rgb[0 * n + j]; t.c1 = rgb[1 * n + j]; t.c2 = rgb[2 * n + j]; t.c3 = rgb[3 * n + j]; t.c4 = rgb[4 * n + j];
  t.f0 = frame[0 * n + j]; t.f1 = frame[1 * n + j]; t.f2 = frame[2 * n + j]; t.f3 = frame[3 * n + j]; t.f4 = frame[4 * n + j];
  t.count = count[j];
  const int64_t o = perm[j];
  if constexpr (kLabel) {
    uint32_t bad = 0u;
    label_word[o] = t.labels(bad);
    if (bad) label_word[n] = 1u;
  }
  // (finalise reads the low 24 bits of a listed view's word and nothing of an empty slot's)
  auto gained = [&](uint32_t c, int32_t f) -> uint32_t {
    if (f < 0) return c;
    const float g = gains[f];
    return (gained_channel((c >> 16) & 0xffu, g) << 16) | (gained_channel((c >> 8) & 0xffu, g) << 8) | gained_channel(c & 0xffu, g);
  };
  t.c0 = gained(t.c0, t.f0);
  t.c1 = gained(t.c1, t.f1);
  t.c2 = gained(t.c2, t.f2);
  t.c3 = gained(t.c3, t.f3);
  t.c4 = gained(t.c4, t.f4);
  rgba[o] = t.finalise();
}

hipError_t preload_exposure() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_pair_stats));
}

int finalise_gained(pcp_context *ctx, uint32_t *result) {
  const int64_t n = ctx->n;
  const uint32_t blocks = static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kExBlock)));
  LaunchTimer t(ctx, PCP_K_MISC);
  if (ctx->label_fusion)
    hipLaunchKernelGGL(k_finalise_gained<true>, dim3(blocks), dim3(kExBlock), 0, ctx->stream, n, ctx->top_score.p, ctx->top_rgb.p,
                       ctx->top_frame.p, ctx->view_count.p, ctx->perm.p, ctx->gains_dev.p, result, ctx->labels.p);
  else
    hipLaunchKernelGGL(k_finalise_gained<false>, dim3(blocks), dim3(kExBlock), 0, ctx->stream, n, ctx->top_score.p, ctx->top_rgb.p,
                       ctx->top_frame.p, ctx->view_count.p, ctx->perm.p, ctx->gains_dev.p, result, static_cast<uint32_t *>(nullptr));
  PCP_HIP_TRY(ctx, hipGetLastError());
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_view_pair_stats(pcp_context *ctx, uint64_t *out_n, uint64_t *out_sum) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!ctx->colour_state_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_view_pair_stats: no top-5 accumulation is live (call it after pcp_colour_pass and "
                     "before pcp_colour_reset)");
  const int32_t F = ctx->n_frames;
  if (F > kExMaxFrames)
    return set_error(ctx, PCP_ERR_RANGE, "pcp_view_pair_stats: %d keyframes (the pair matrices are built for up to %d)", F, kExMaxFrames);
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t cells = static_cast<size_t>(F) * static_cast<size_t>(F);
  int32_t table_log2 = kExTableLog2;
  if (const char *e = std::getenv("PCP_EXPOSURE_TABLE_LOG2"))  // read per call: the tests shrink the table inside one process
    table_log2 = std::min(kExTableLog2, std::max(0, std::atoi(e)));
  PCP_HIP_TRY(ctx, ctx->pair_stats.ensure(2 * cells + 4));
  unsigned long long *d_n = ctx->pair_stats.p, *d_sum = d_n + cells, *d_counters = d_sum + cells;
  PCP_HIP_TRY(ctx, hipMemsetAsync(d_n, 0, (2 * cells + 4) * 8, ctx->stream));
  const int64_t n = ctx->n;
  if (n > 0) {
    const uint32_t blocks = static_cast<uint32_t>(std::min<int64_t>(div_up(n, kExBlock), kExMaxGrid));
    const size_t lds = (4u * (size_t(1) << table_log2) + 3u) * sizeof(uint32_t);
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_pair_stats, dim3(blocks), dim3(kExBlock), lds, ctx->stream, n, ctx->top_rgb.p, ctx->top_frame.p,
                       static_cast<uint32_t>(F), table_log2, d_n, d_sum, d_counters);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit counters");
  if (out_n && cells) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_n, d_n, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out_sum && cells) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_sum, d_sum, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
  unsigned long long h[4] = {0, 0, 0, 0};
  PCP_HIP_TRY(ctx, hipMemcpyAsync(h, d_counters, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 4; ++k) ctx->pair_counters[k] = static_cast<int64_t>(h[k]);
  ctx->pair_counters[4] = int64_t(1) << table_log2;
  ctx->pair_counters_live = true;
  return PCP_OK;
}

int pcp_view_pair_stats_counters(pcp_context *ctx, int64_t out[5]) {
  if (!ctx || !out) return PCP_ERR_INVALID;
  if (!ctx->pair_counters_live) return set_error(ctx, PCP_ERR_STATE, "pcp_view_pair_stats_counters: pcp_view_pair_stats has not run");
  for (int k = 0; k < 5; ++k) out[k] = ctx->pair_counters[k];
  return PCP_OK;
}

int pcp_exposure_gains(int32_t n_frames, const uint64_t *n, const uint64_t *sum, double sigma_n, double sigma_g, double *out_gains) {
  if (n_frames < 1 || !n || !sum || !out_gains) {
    set_global_error("pcp_exposure_gains: %d keyframes / a NULL argument", n_frames);
    return PCP_ERR_INVALID;
  }
  if (n_frames > kExMaxFrames) {
    set_global_error("pcp_exposure_gains: %d keyframes (the dense solve is built for up to %d)", n_frames, kExMaxFrames);
    return PCP_ERR_RANGE;
  }
  if (!(std::isfinite(sigma_n) && sigma_n > 0.0 && std::isfinite(sigma_g) && sigma_g > 0.0)) {
    set_global_error("pcp_exposure_gains: sigma_n %g, sigma_g %g (both must be finite and positive)", sigma_n, sigma_g);
    return PCP_ERR_INVALID;
  }
  const size_t F = static_cast<size_t>(n_frames);
  for (size_t i = 0; i < F; ++i)
    for (size_t j = 0; j < F; ++j) {
      if (n[i * F + j] != n[j * F + i]) {
        set_global_error("pcp_exposure_gains: n[%zu][%zu] != n[%zu][%zu] (every pair is counted in both orders)", i, j, j, i);
        return PCP_ERR_INVALID;
      }
      if (n[i * F + j] > (~uint64_t(0)) / 255u || sum[i * F + j] > 255u * n[i * F + j]) {
        set_global_error("pcp_exposure_gains: sum[%zu][%zu] exceeds 255 n[%zu][%zu]", i, j, i, j);
        return PCP_ERR_INVALID;
      }
    }
  // EG4: the active set (keyframes with a pair), the normal equations, a dense Cholesky in a fixed order
  std::vector<int32_t> active;
  for (size_t i = 0; i < F; ++i) {
    bool any = false;
    for (size_t j = 0; j < F && !any; ++j) any = j != i && n[i * F + j] != 0;
    out_gains[i] = 1.0;
    if (any) active.push_back(static_cast<int32_t>(i));
  }
  const size_t m = active.size();
  if (m == 0) return PCP_OK;
  std::vector<double> A, b;
  try {
    A.assign(m * m, 0.0);
    b.assign(m, 0.0);
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_exposure_gains: out of host memory for a %zu x %zu system", m, m);
    return PCP_ERR_NOMEM;
  }
  const double wn = 1.0 / (sigma_n * sigma_n), wg = 1.0 / (sigma_g * sigma_g);
  for (size_t r = 0; r < m; ++r) {
    const size_t i = static_cast<size_t>(active[r]);
    for (size_t c = 0; c < m; ++c) {
      const size_t j = static_cast<size_t>(active[c]);
      const uint64_t nij = n[i * F + j];
      if (j == i || nij == 0) continue;
      const double w = static_cast<double>(nij);
      const double iij = static_cast<double>(sum[i * F + j]) / w, iji = static_cast<double>(sum[j * F + i]) / w;
      A[r * m + r] += w * (iij * iij * wn + wg);
      A[r * m + c] -= w * iij * iji * wn;
      b[r] += w * wg;
    }
  }
  // A = L L^T, row by row (the lower triangle of A becomes L); the dot products run in index order in four interleaved
  // partial sums that are added in a fixed order: the same bits on every run
  auto dot = [](const double *p, const double *q, size_t len) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    size_t k = 0;
    for (; k + 4 <= len; k += 4) {
      s0 += p[k] * q[k];
      s1 += p[k + 1] * q[k + 1];
      s2 += p[k + 2] * q[k + 2];
      s3 += p[k + 3] * q[k + 3];
    }
    for (; k < len; ++k) s0 += p[k] * q[k];
    return (s0 + s1) + (s2 + s3);
  };
  for (size_t r = 0; r < m; ++r) {
    for (size_t c = 0; c < r; ++c) A[r * m + c] = (A[r * m + c] - dot(&A[r * m], &A[c * m], c)) / A[c * m + c];
    const double d = A[r * m + r] - dot(&A[r * m], &A[r * m], r);
    if (!(d > 0.0) || !std::isfinite(d)) {
      set_global_error("pcp_exposure_gains: the system is not positive definite at keyframe %d (pivot %g)", active[r], d);
      return PCP_ERR_RANGE;
    }
    A[r * m + r] = std::sqrt(d);
  }
  for (size_t r = 0; r < m; ++r) b[r] = (b[r] - dot(&A[r * m], b.data(), r)) / A[r * m + r];  // L z = b
  for (size_t r = m; r-- > 0;) {                                                                // L^T g = z
    double s = b[r];
    for (size_t k = r + 1; k < m; ++k) s -= A[k * m + r] * b[k];
    b[r] = s / A[r * m + r];
  }
  for (size_t r = 0; r < m; ++r) out_gains[static_cast<size_t>(active[r])] = b[r];
  return PCP_OK;
}

int pcp_set_frame_gains(pcp_context *ctx, const double *gains, int32_t n) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!gains) {
    ctx->gains_set = false;
    return PCP_OK;
  }
  if (n != ctx->n_frames || n < 1)
    return set_error(ctx, PCP_ERR_INVALID, "pcp_set_frame_gains: %d gains for %d keyframes", n, ctx->n_frames);
  for (int32_t f = 0; f < n; ++f)
    if (!(std::isfinite(gains[f]) && gains[f] > 0.0 && gains[f] <= 16.0))
      return set_error(ctx, PCP_ERR_INVALID, "pcp_set_frame_gains: gain %g of keyframe %d outside (0, 16]", gains[f], f);
  std::vector<float> g32(static_cast<size_t>(n));
  for (int32_t f = 0; f < n; ++f) g32[static_cast<size_t>(f)] = static_cast<float>(gains[f]);
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (a finalise queued under the previous gains may still read the buffer: the copy is ordered behind it on the stream)
  PCP_HIP_TRY(ctx, ctx->gains_dev.ensure(static_cast<size_t>(n) + 4));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(ctx->gains_dev.p, g32.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->gains_set = true;
  return PCP_OK;
}

}  // extern "C"
