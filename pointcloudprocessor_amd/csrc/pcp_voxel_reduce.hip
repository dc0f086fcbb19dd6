// pcp_voxel_reduce.hip -- voxel-grid reduction of the coloured cloud ("Voxel-grid output", VG1-VG7): one row per
// occupied voxel of edge `leaf` -- centroid, mean colour, mean fused label, row count -- accumulated on the device over any
// number of colour results (one-shot runs, index shards, the chunks of the streamed chain).  The arithmetic is
// pcp_voxel_reduce.hpp's, exact integers, so the result does not depend on the order of rows, chunks or atomics.
//
// The accumulator is an open-addressing table in device memory: 64-bit keys placed by compare-and-swap, payloads (three
// signed 64-bit position sums; n, r, g, b, label as 32-bit sums) updated by integer atomic adds only.  Every add runs two
// passes over the rows: pass A places keys only (idempotent; it also finds every refusal), pass B adds payloads (every key
// is present, nothing can overflow).  A pass A that fails or finds the table too small therefore leaves no payload behind.
// Opt-in: nothing here runs unless one of its entry points is called.
#include <algorithm>
#include <new>
#include <utility>
#include <vector>

#include "pcp_internal.hpp"
#include "pcp_scan.hpp"
#include "pcp_voxel_reduce.hpp"

namespace pcp {

constexpr int kVrBlock = 256;
constexpr int64_t kVrMaxGrid = 4096;          // workgroups of the grid-stride passes
constexpr int64_t kVrMinSlots = 64;           // (the tests start there to walk the growth)
constexpr int64_t kVrMaxSlots = int64_t(1) << 31;
constexpr int64_t kVrDefaultMinSlots = int64_t(1) << 16;
constexpr uint32_t kVrMaxProbes = 1024;       // linear probes of pass A before it asks for a larger table
// device scalars of the accumulator
enum { VR_USED = 0, VR_ROWS, VR_RANGE, VR_MISSED, VR_PARTIALS, VR_ATOMICS, VR_COMPACTED, VR_CROWDED, VR_SCALARS };

struct VrTable {
  unsigned long long *keys;  // [slots]
  unsigned long long *q;     // [3][slots]: sums of the offsets from the corner, two's complement
  uint32_t *sums;            // [5][slots]: n, r, g, b, label
  uint64_t mask;             // slots - 1
  int32_t shift;             // 64 - log2(slots)
};

__device__ __forceinline__ uint64_t vr_home(const VrTable &t, uint64_t key) {
  return t.shift < 64 ? (key * 0x9e3779b97f4a7c15ull) >> t.shift : 0ull;
}

// the key of row j of the upload's spatial order (sxyz / perm, the Hilbert-sorted planes: the uploaded coordinates; the packed
// word and the has bit of the input-order result); kNoKey: no row / no colour.  *bad: a coordinate VG3 refuses.
__device__ __forceinline__ uint64_t vr_row_key(int64_t j, int64_t n, const float *__restrict__ sx, const float *__restrict__ sy,
                                               const float *__restrict__ sz, const int32_t *__restrict__ perm,
                                               const uint32_t *__restrict__ packed, float inv, int32_t *row, uint32_t *word, bool *bad) {
  *bad = false;
  if (j >= n) return vg::kNoKey;
  const int32_t i = perm[j];
  const uint32_t w = packed[i];
  if (!(w >> 24)) return vg::kNoKey;
  int32_t cx, cy, cz;
  const bool ok = vg::cell_of(sx[j], inv, &cx) & vg::cell_of(sy[j], inv, &cy) & vg::cell_of(sz[j], inv, &cz);
  if (!ok) {
    *bad = true;
    return vg::kNoKey;
  }
  *row = i;
  *word = w;
  return vg::key_of(cx, cy, cz);
}

// a lane without a row takes the key of the nearest lane below that has one (and adds nothing): rows without a colour then do
// not cut a run of equal keys in two
__device__ __forceinline__ uint64_t vr_bridge_gaps(uint64_t key, int lane) {
  const unsigned long long with_key = __ballot(key != vg::kNoKey);
  const unsigned long long below = with_key & ((1ull << lane) - 1ull);
  const int src = (key == vg::kNoKey && below) ? 63 - __clzll(static_cast<long long>(below)) : lane;
  return __shfl(static_cast<unsigned long long>(key), src, 64);
}

// Pass A.  One lane per row, in the upload's spatial order: neighbouring lanes share voxels, and only the first lane of a run of equal keys
// places the key.  A key is placed once whatever the number of adds that carry it, so the pass can be repeated.  When the
// table fills past 3/4 or a key finds no place within kVrMaxProbes the pass raises VR_MISSED and the wavefronts stop at
// their next tile: the host grows the table and runs the pass again.
__global__ __launch_bounds__(kVrBlock) void k_vr_insert(int64_t n, const float *__restrict__ sx, const float *__restrict__ sy,
                                                        const float *__restrict__ sz, const int32_t *__restrict__ perm,
                                                        const uint32_t *__restrict__ packed, float inv, VrTable t,
                                                        unsigned long long *__restrict__ scalars) {
  const int lane = static_cast<int>(threadIdx.x & 63u);
  const uint64_t slots = t.mask + 1ull;
  const uint32_t probes = static_cast<uint32_t>(slots < kVrMaxProbes ? slots : kVrMaxProbes);
  uint32_t rows = 0u;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kVrBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kVrBlock) {
    // (one load per wavefront instruction: the value is the same in its lanes; made explicit for the shuffle below)
    const unsigned long long stop = *reinterpret_cast<volatile unsigned long long *>(scalars + VR_MISSED);
    if (__builtin_amdgcn_readfirstlane(static_cast<int>(stop != 0ull))) break;
    int32_t row = 0;
    uint32_t word = 0u;
    bool bad;
    const uint64_t key = vr_row_key(base + threadIdx.x, n, sx, sy, sz, perm, packed, inv, &row, &word, &bad);
    if (bad) atomicOr(scalars + VR_RANGE, 1ull);
    rows += key != vg::kNoKey ? 1u : 0u;
    const uint64_t run_key = vr_bridge_gaps(key, lane);
    const uint64_t before = __shfl_up(static_cast<unsigned long long>(run_key), 1, 64);
    const bool head = run_key != vg::kNoKey && (lane == 0 || before != run_key);  // (a head is a lane with a row of its own)
    if (head) {
      const uint64_t home = vr_home(t, key);
      bool placed = false;
      for (uint32_t p = 0; p < probes && !placed; ++p) {
        const uint64_t s = (home + p) & t.mask;
        // (a key never changes once placed: a plain load that shows another key is final, one that shows none is confirmed by the swap)
        unsigned long long cur = t.keys[s];
        if (cur == vg::kNoKey) {
          cur = atomicCAS(t.keys + s, static_cast<unsigned long long>(vg::kNoKey), static_cast<unsigned long long>(key));
          if (cur == vg::kNoKey) {
            const unsigned long long used = atomicAdd(scalars + VR_USED, 1ull) + 1ull;
            if (used * 4ull > slots * 3ull) atomicOr(scalars + VR_MISSED, 1ull);
            placed = true;
          }
        }
        if (cur == key) placed = true;
      }
      if (!placed) atomicOr(scalars + VR_MISSED, 1ull);
    }
  }
  if (rows) atomicAdd(scalars + VR_ROWS, static_cast<unsigned long long>(rows));
}

// Pass B.  The rows of a run of equal keys among neighbouring lanes are summed inside the wavefront (a segmented suffix sum
// over the run: six shuffle steps, exact integers) and the run's first lane issues one set of adds: three 64-bit position
// sums and four (five with labels) 32-bit sums.  n, r (and g, b) travel as 16-bit halves of one word: 64 lanes x 255 < 2^16.
template <bool kLabel>
__global__ __launch_bounds__(kVrBlock) void k_vr_accumulate(int64_t n, const float *__restrict__ sx, const float *__restrict__ sy,
                                                            const float *__restrict__ sz, const int32_t *__restrict__ perm,
                                                            const uint32_t *__restrict__ packed,
                                                            [[maybe_unused]] const uint32_t *__restrict__ labels, float leaf, float inv,
                                                            VrTable t, unsigned long long *__restrict__ scalars) {
  const int lane = static_cast<int>(threadIdx.x & 63u);
  const uint64_t slots = t.mask + 1ull;
  uint32_t partials = 0u;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kVrBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kVrBlock) {
    const int64_t j = base + threadIdx.x;
    int32_t row = 0;
    uint32_t word = 0u;
    bool bad;
    const uint64_t key = vr_row_key(j, n, sx, sy, sz, perm, packed, inv, &row, &word, &bad);
    long long q0 = 0, q1 = 0, q2 = 0;
    uint32_t nr = 0u, gb = 0u, lab = 0u;
    if (key != vg::kNoKey) {
      int32_t cx, cy, cz;
      vg::cells_of_key(key, &cx, &cy, &cz);
      q0 = vg::fixed_of(sx[j]) - vg::corner_of(cx, leaf);
      q1 = vg::fixed_of(sy[j]) - vg::corner_of(cy, leaf);
      q2 = vg::fixed_of(sz[j]) - vg::corner_of(cz, leaf);
      nr = 1u | ((word & 0xffu) << 16);
      gb = ((word >> 8) & 0xffu) | (((word >> 16) & 0xffu) << 16);
      if constexpr (kLabel) lab = labels[row] & 0xffu;
    }
    const uint64_t run_key = vr_bridge_gaps(key, lane);
    const uint64_t before = __shfl_up(static_cast<unsigned long long>(run_key), 1, 64);
    const bool head = lane == 0 || before != run_key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int run_end = above ? lane + (__ffsll(above) - 1) : 63;  // last lane of this lane's run
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long t0 = __shfl_down(q0, d, 64), t1 = __shfl_down(q1, d, 64), t2 = __shfl_down(q2, d, 64);
      const uint32_t tn = __shfl_down(nr, d, 64), tg = __shfl_down(gb, d, 64);
      uint32_t tl = 0u;
      if constexpr (kLabel) tl = __shfl_down(lab, d, 64);
      if (lane + d <= run_end) {
        q0 += t0;
        q1 += t1;
        q2 += t2;
        nr += tn;
        gb += tg;
        lab += tl;
      }
    }
    if (head && run_key != vg::kNoKey) {  // (such a head is a lane with a row of its own: key == run_key)
      const uint64_t home = vr_home(t, key);
      uint64_t s = home;
      bool found = false;
      for (uint64_t p = 0; p < slots && !found; ++p) {  // (pass A placed every key: the walk ends at it)
        s = (home + p) & t.mask;
        found = t.keys[s] == key;
      }
      if (found) {
        atomicAdd(t.q + s, static_cast<unsigned long long>(q0));
        atomicAdd(t.q + slots + s, static_cast<unsigned long long>(q1));
        atomicAdd(t.q + 2 * slots + s, static_cast<unsigned long long>(q2));
        atomicAdd(t.sums + s, nr & 0xffffu);
        atomicAdd(t.sums + slots + s, nr >> 16);
        atomicAdd(t.sums + 2 * slots + s, gb & 0xffffu);
        atomicAdd(t.sums + 3 * slots + s, gb >> 16);
        if constexpr (kLabel) atomicAdd(t.sums + 4 * slots + s, lab);
        partials += 1u;
      } else {
        atomicOr(scalars + VR_MISSED, 1ull);
      }
    }
  }
  if (partials) {
    atomicAdd(scalars + VR_PARTIALS, static_cast<unsigned long long>(partials));
    atomicAdd(scalars + VR_ATOMICS, static_cast<unsigned long long>(partials) * (kLabel ? 8ull : 7ull));
  }
}

__global__ __launch_bounds__(kVrBlock) void k_vr_fill64(unsigned long long *__restrict__ p, int64_t n, unsigned long long v) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * kVrBlock + threadIdx.x;
  for (; i < n; i += static_cast<int64_t>(gridDim.x) * kVrBlock) p[i] = v;
}

// every key of `from` (with keep_empty == 0: every key that holds a row) into the cleared table `to`, payload and all: the
// keys of a table are distinct, so each finds a slot of its own and plain stores move the payload
__global__ __launch_bounds__(kVrBlock) void k_vr_rehash(VrTable from, VrTable to, int32_t keep_empty,
                                                        unsigned long long *__restrict__ scalars) {
  const int64_t old_slots = static_cast<int64_t>(from.mask + 1ull), new_slots = static_cast<int64_t>(to.mask + 1ull);
  uint32_t moved = 0u;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kVrBlock + threadIdx.x; s < old_slots; s += static_cast<int64_t>(gridDim.x) * kVrBlock) {
    const unsigned long long key = from.keys[s];
    if (key == vg::kNoKey) continue;
    const uint32_t rows = from.sums[s];
    if (!keep_empty && rows == 0u) continue;
    const uint64_t home = vr_home(to, key);
    int64_t d = -1;
    for (int64_t p = 0; p < new_slots && d < 0; ++p) {
      const uint64_t c = (home + static_cast<uint64_t>(p)) & to.mask;
      if (atomicCAS(to.keys + c, static_cast<unsigned long long>(vg::kNoKey), key) == vg::kNoKey) d = static_cast<int64_t>(c);
    }
    if (d < 0) {  // (the new table is at least as large as the old one: not reached)
      atomicOr(scalars + VR_MISSED, 1ull);
      continue;
    }
    for (int a = 0; a < 3; ++a) to.q[a * new_slots + d] = from.q[a * old_slots + s];
    for (int a = 0; a < 5; ++a) to.sums[a * new_slots + d] = from.sums[a * old_slots + s];
    moved += 1u;
  }
  if (moved) atomicAdd(scalars + VR_USED, static_cast<unsigned long long>(moved));
}

// the slots that hold rows, in any order (the sort orders them): key and slot
__global__ __launch_bounds__(kVrBlock) void k_vr_compact(VrTable t, unsigned long long *__restrict__ out_key, int32_t *__restrict__ out_slot,
                                                         int64_t capacity, unsigned long long *__restrict__ scalars) {
  const int64_t slots = static_cast<int64_t>(t.mask + 1ull);
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kVrBlock + threadIdx.x; s < slots; s += static_cast<int64_t>(gridDim.x) * kVrBlock) {
    const unsigned long long key = t.keys[s];
    if (key == vg::kNoKey) continue;
    const uint32_t rows = t.sums[s];
    if (rows == 0u) continue;
    if (rows >= vg::kMaxRowsPerVoxel) atomicOr(scalars + VR_CROWDED, 1ull);
    const int64_t pos = static_cast<int64_t>(atomicAdd(scalars + VR_COMPACTED, 1ull));
    if (pos < capacity) {
      out_key[pos] = key;
      out_slot[pos] = static_cast<int32_t>(s);
    }
  }
}

// LSD radix sort of (63-bit key, slot): pcp_context.hip's passes over 64-bit keys
__global__ __launch_bounds__(kVrBlock) void k_vr_radix_hist(const unsigned long long *__restrict__ key, int64_t n, int32_t shift,
                                                            int32_t *__restrict__ hist, int64_t blocks) {
  __shared__ int32_t cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kVrBlock + threadIdx.x;
  if (i < n) atomicAdd(&cnt[(key[i] >> shift) & 0xffull], 1);
  __syncthreads();
  hist[static_cast<int64_t>(threadIdx.x) * blocks + blockIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(kVrBlock) void k_vr_radix_scatter(const unsigned long long *__restrict__ key_in, const int32_t *__restrict__ val_in,
                                                               int64_t n, int32_t shift, const int32_t *__restrict__ offs, int64_t blocks,
                                                               unsigned long long *__restrict__ key_out, int32_t *__restrict__ val_out) {
  __shared__ int32_t wcount[kVrBlock / 64][256];
  __shared__ int32_t wbase[kVrBlock / 64][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = 0; k < kVrBlock / 64; ++k) wcount[k][threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kVrBlock + threadIdx.x;
  const bool valid = i < n;
  const unsigned long long k = valid ? key_in[i] : 0ull;
  const int32_t v = valid ? val_in[i] : 0;
  const uint32_t digit = static_cast<uint32_t>((k >> shift) & 0xffull);
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  const int rank = __popcll(peers & ((1ull << lane) - 1ull));
  if (valid && rank == 0) wcount[wave][digit] = __popcll(peers);
  __syncthreads();
  {
    int32_t run = offs[static_cast<int64_t>(threadIdx.x) * blocks + blockIdx.x];  // this thread = one digit
    for (int w = 0; w < kVrBlock / 64; ++w) {
      wbase[w][threadIdx.x] = run;
      run += wcount[w][threadIdx.x];
    }
  }
  __syncthreads();
  if (valid) {
    const int64_t pos = static_cast<int64_t>(wbase[wave][digit]) + rank;
    if (pos < n) {
      key_out[pos] = k;
      val_out[pos] = v;
    }
  }
}

// VG7 over the sorted slots
__global__ __launch_bounds__(kVrBlock) void k_vr_finish(int64_t voxels, const unsigned long long *__restrict__ key, const int32_t *__restrict__ slot,
                                                        VrTable t, float leaf, float *__restrict__ out_xyz, uint8_t *__restrict__ out_rgb,
                                                        uint8_t *__restrict__ out_label, uint32_t *__restrict__ out_count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kVrBlock + threadIdx.x;
  if (i >= voxels) return;
  const int64_t slots = static_cast<int64_t>(t.mask + 1ull);
  const int64_t s = slot[i];
  vg::Sums sums;
  for (int a = 0; a < 3; ++a) sums.q[a] = static_cast<int64_t>(t.q[a * slots + s]);
  sums.n = t.sums[s];
  sums.r = t.sums[slots + s];
  sums.g = t.sums[2 * slots + s];
  sums.b = t.sums[3 * slots + s];
  sums.label = t.sums[4 * slots + s];
  float xyz[3];
  uint8_t rgb[3], label;
  vg::finish_voxel(key[i], leaf, sums, xyz, rgb, &label);
  for (int a = 0; a < 3; ++a) {
    out_xyz[3 * i + a] = xyz[a];
    out_rgb[3 * i + a] = rgb[a];
  }
  out_label[i] = label;
  out_count[i] = sums.n;
}

hipError_t preload_voxel_reduce() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_vr_insert));
}

static inline uint32_t vr_blocks(int64_t n) {
  return static_cast<uint32_t>(std::max<int64_t>(1, std::min<int64_t>(div_up(n, kVrBlock), kVrMaxGrid)));
}
static inline int64_t pow2_at_least(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

static VrTable vr_view(unsigned long long *keys, unsigned long long *q, uint32_t *sums, int64_t slots) {
  VrTable t;
  t.keys = keys;
  t.q = q;
  t.sums = sums;
  t.mask = static_cast<uint64_t>(slots) - 1ull;
  int32_t log2 = 0;
  while ((int64_t(1) << log2) < slots) ++log2;
  t.shift = 64 - log2;
  return t;
}
static VrTable vr_table(pcp_context *ctx) {
  VoxelReduce &vr = ctx->voxel_reduce;
  return vr_view(vr.keys.p, vr.q.p, vr.sums.p, vr.slots);
}

// a cleared table of `slots` slots in (keys, q, sums)
static int vr_clear(pcp_context *ctx, DevBuf<unsigned long long> &keys, DevBuf<unsigned long long> &q, DevBuf<uint32_t> &sums, int64_t slots) {
  const size_t s = static_cast<size_t>(slots);
  PCP_HIP_TRY(ctx, keys.ensure(s + 2));
  PCP_HIP_TRY(ctx, q.ensure(3 * s + 2));
  PCP_HIP_TRY(ctx, sums.ensure(5 * s + 4));
  LaunchTimer t(ctx, PCP_K_MISC);
  hipLaunchKernelGGL(k_vr_fill64, dim3(vr_blocks(slots)), dim3(kVrBlock), 0, ctx->stream, keys.p, slots, static_cast<unsigned long long>(vg::kNoKey));
  PCP_HIP_TRY(ctx, hipGetLastError());
  PCP_HIP_TRY(ctx, hipMemsetAsync(q.p, 0, 3 * s * 8, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(sums.p, 0, 5 * s * 4, ctx->stream));
  return PCP_OK;
}

static int vr_read_scalars(pcp_context *ctx, unsigned long long h[VR_SCALARS]) {
  PCP_HIP_TRY(ctx, hipMemcpyAsync(h, ctx->voxel_reduce.scalars.p, VR_SCALARS * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

// the table's keys (those that hold rows, or all of them) into a fresh table of new_slots slots
static int vr_rehash(pcp_context *ctx, int64_t new_slots, bool keep_empty) {
  VoxelReduce &vr = ctx->voxel_reduce;
  DevBuf<unsigned long long> keys, q;
  DevBuf<uint32_t> sums;  // (whichever table is not the accumulator's is freed on return)
  int rc = vr_clear(ctx, keys, q, sums, new_slots);
  if (rc != PCP_OK) return rc;
  PCP_HIP_TRY(ctx, hipMemsetAsync(vr.scalars.p + VR_USED, 0, 8, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemsetAsync(vr.scalars.p + VR_MISSED, 0, 8, ctx->stream));
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_vr_rehash, dim3(vr_blocks(vr.slots)), dim3(kVrBlock), 0, ctx->stream, vr_table(ctx),
                       vr_view(keys.p, q.p, sums.p, new_slots), keep_empty ? 1 : 0, vr.scalars.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  unsigned long long h[VR_SCALARS];
  if ((rc = vr_read_scalars(ctx, h)) != PCP_OK) return rc;
  if (h[VR_MISSED]) return set_error(ctx, PCP_ERR_DEVICE, "pcp_voxel_reduce: a key found no slot while the table was rebuilt");
  std::swap(vr.keys, keys);
  std::swap(vr.q, q);
  std::swap(vr.sums, sums);
  vr.slots = new_slots;
  vr.used = static_cast<int64_t>(h[VR_USED]);
  return PCP_OK;
}

static void vr_drop(pcp_context *ctx) {
  VoxelReduce &vr = ctx->voxel_reduce;
  vr.keys.release();
  vr.q.release();
  vr.sums.release();
  vr.scalars.release();
  vr.out_xyz.release();
  vr.out_rgb.release();
  vr.out_label.release();
  vr.out_count.release();
  vr.live = vr.finished = vr.labels_fixed = vr.with_label = false;
  vr.slots = vr.used = vr.keyed = vr.rows = vr.voxels = vr.growths = vr.partials = vr.atomics = 0;
  vr.initial_slots = 0;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_voxel_reduce_begin(pcp_context *ctx, float leaf, int64_t initial_slots) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!vg::leaf_ok(leaf)) return set_error(ctx, PCP_ERR_INVALID, "pcp_voxel_reduce_begin: leaf %g outside [1e-4, 1]", static_cast<double>(leaf));
  if (initial_slots < 0 || initial_slots > kVrMaxSlots)
    return set_error(ctx, PCP_ERR_INVALID, "pcp_voxel_reduce_begin: initial_slots %lld outside 0..2^31", static_cast<long long>(initial_slots));
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vr_drop(ctx);
  VoxelReduce &vr = ctx->voxel_reduce;
  PCP_HIP_TRY(ctx, vr.scalars.ensure(VR_SCALARS));
  PCP_HIP_TRY(ctx, hipMemsetAsync(vr.scalars.p, 0, VR_SCALARS * 8, ctx->stream));
  vr.leaf = leaf;
  vr.initial_slots = initial_slots ? pow2_at_least(std::max(initial_slots, kVrMinSlots)) : 0;  // 0: sized by the first add
  vr.live = true;
  return PCP_OK;
}

int pcp_voxel_reduce_add(pcp_context *ctx, int64_t *out_rows_added) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows_added) *out_rows_added = 0;
  VoxelReduce &vr = ctx->voxel_reduce;
  if (!vr.live) return set_error(ctx, PCP_ERR_STATE, "pcp_voxel_reduce_add: no accumulation (call pcp_voxel_reduce_begin)");
  if (vr.finished) return set_error(ctx, PCP_ERR_STATE, "pcp_voxel_reduce_add: the accumulation is finished (pcp_voxel_reduce_begin starts the next)");
  if (!ctx->colour_result_live)
    return set_error(ctx, PCP_ERR_STATE, "pcp_voxel_reduce_add: no colour result (call pcp_colorize / pcp_colorize_from_depth / pcp_colour_finalise)");
  const bool with_label = ctx->labels_live;
  if (vr.labels_fixed && with_label != vr.with_label)
    return set_error(ctx, PCP_ERR_STATE, "pcp_voxel_reduce_add: this colour result was made %s label fusion, the accumulation's first %s it",
                     with_label ? "with" : "without", vr.with_label ? "with" : "without");
  const int64_t n = ctx->n;
  if (n == 0) {
    vr.labels_fixed = true;
    vr.with_label = with_label;
    return PCP_OK;
  }
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if (vr.slots == 0) {
    const int64_t slots = vr.initial_slots ? vr.initial_slots : std::min(kVrMaxSlots, pow2_at_least(std::max(kVrDefaultMinSlots, n / 4)));
    if ((rc = vr_clear(ctx, vr.keys, vr.q, vr.sums, slots)) != PCP_OK) return rc;
    vr.slots = slots;
    vr.used = 0;
  }
  const size_t plane = (static_cast<size_t>(n) + 3) & ~size_t(3);
  const float *sx = ctx->sxyz.p, *sy = sx + plane, *sz = sy + plane;
  const uint32_t *packed = ctx->rgba2[ctx->rgba_cur].p;
  const float inv = vg::inverse_leaf(vr.leaf);
  unsigned long long h[VR_SCALARS];
  for (;;) {  // pass A, again after every growth that it asked for
    PCP_HIP_TRY(ctx, hipMemsetAsync(vr.scalars.p + VR_ROWS, 0, 3 * 8, ctx->stream));  // rows, range, missed
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_vr_insert, dim3(vr_blocks(n)), dim3(kVrBlock), 0, ctx->stream, n, sx, sy, sz, ctx->perm.p, packed, inv,
                         vr_table(ctx), vr.scalars.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    if ((rc = vr_read_scalars(ctx, h)) != PCP_OK) return rc;
    vr.used = static_cast<int64_t>(h[VR_USED]);
    if (h[VR_RANGE]) {
      // the keys this call placed hold no row: the table without them is the table as it was
      if ((rc = vr_rehash(ctx, vr.slots, false)) != PCP_OK) return rc;
      return set_error(ctx, PCP_ERR_RANGE, "pcp_voxel_reduce_add: a coloured row has a non-finite coordinate or lies %g m or more from the "
                       "origin on an axis (2^20 leaves of %g m); nothing was added", 1048576.0 * static_cast<double>(vr.leaf),
                       static_cast<double>(vr.leaf));
    }
    if (!h[VR_MISSED] && vr.used * 2 <= vr.slots) break;
    int64_t want = vr.slots;
    while (want < 4 * vr.used || want <= vr.slots) want <<= 1;
    if (want > kVrMaxSlots) {
      if ((rc = vr_rehash(ctx, vr.slots, false)) != PCP_OK) return rc;
      return set_error(ctx, PCP_ERR_RANGE, "pcp_voxel_reduce_add: more than 2^30 occupied voxels; nothing was added");
    }
    for (int64_t s = vr.slots; s < want; s <<= 1) vr.growths += 1;  // counted in doublings
    const bool again = h[VR_MISSED] != 0;
    if ((rc = vr_rehash(ctx, want, true)) != PCP_OK) return rc;
    if (!again) break;
  }
  const int64_t rows = static_cast<int64_t>(h[VR_ROWS]);
  PCP_HIP_TRY(ctx, hipMemsetAsync(vr.scalars.p + VR_MISSED, 0, 3 * 8, ctx->stream));  // missed, partials, atomics
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    if (with_label)
      hipLaunchKernelGGL(k_vr_accumulate<true>, dim3(vr_blocks(n)), dim3(kVrBlock), 0, ctx->stream, n, sx, sy, sz, ctx->perm.p, packed,
                         ctx->labels.p, vr.leaf, inv, vr_table(ctx), vr.scalars.p);
    else
      hipLaunchKernelGGL(k_vr_accumulate<false>, dim3(vr_blocks(n)), dim3(kVrBlock), 0, ctx->stream, n, sx, sy, sz, ctx->perm.p, packed,
                         static_cast<const uint32_t *>(nullptr), vr.leaf, inv, vr_table(ctx), vr.scalars.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  if ((rc = vr_read_scalars(ctx, h)) != PCP_OK) return rc;
  if (h[VR_MISSED]) return set_error(ctx, PCP_ERR_DEVICE, "pcp_voxel_reduce_add: a row's key was not in the table");
  vr.partials += static_cast<int64_t>(h[VR_PARTIALS]);
  vr.atomics += static_cast<int64_t>(h[VR_ATOMICS]);
  vr.rows += rows;
  vr.keyed = vr.used;  // (pass B gave every key of the table a row)
  vr.labels_fixed = true;
  vr.with_label = with_label;
  if (out_rows_added) *out_rows_added = rows;
  return PCP_OK;
}

int pcp_voxel_reduce_finish(pcp_context *ctx, int64_t *out_voxels) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_voxels) *out_voxels = 0;
  VoxelReduce &vr = ctx->voxel_reduce;
  if (!vr.live) return set_error(ctx, PCP_ERR_STATE, "pcp_voxel_reduce_finish: no accumulation (call pcp_voxel_reduce_begin)");
  if (vr.finished) {
    if (out_voxels) *out_voxels = vr.voxels;
    return PCP_OK;
  }
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int64_t voxels = 0;
  if (vr.slots > 0 && vr.used > 0) {
    const size_t cap = static_cast<size_t>(vr.used);
    DevBuf<unsigned long long> key_a, key_b;
    DevBuf<int32_t> val_a, val_b, hist;
    PCP_HIP_TRY(ctx, key_a.ensure(cap + 2));
    PCP_HIP_TRY(ctx, key_b.ensure(cap + 2));
    PCP_HIP_TRY(ctx, val_a.ensure(cap + 4));
    PCP_HIP_TRY(ctx, val_b.ensure(cap + 4));
    PCP_HIP_TRY(ctx, hipMemsetAsync(vr.scalars.p + VR_COMPACTED, 0, 2 * 8, ctx->stream));  // compacted, crowded
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_vr_compact, dim3(vr_blocks(vr.slots)), dim3(kVrBlock), 0, ctx->stream, vr_table(ctx), key_a.p, val_a.p,
                         vr.used, vr.scalars.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    unsigned long long h[VR_SCALARS];
    int rc = vr_read_scalars(ctx, h);
    if (rc != PCP_OK) return rc;
    if (h[VR_CROWDED])
      return set_error(ctx, PCP_ERR_RANGE, "pcp_voxel_reduce_finish: a voxel holds 2^24 rows or more (the 32-bit colour sums are built for fewer)");
    voxels = static_cast<int64_t>(h[VR_COMPACTED]);
    if (voxels > vr.used) return set_error(ctx, PCP_ERR_DEVICE, "pcp_voxel_reduce_finish: %lld occupied slots of %lld keys",
                                           static_cast<long long>(voxels), static_cast<long long>(vr.used));
    if (voxels > 0) {
      const int64_t blocks = div_up(voxels, kVrBlock), hm = 256 * blocks;
      PCP_HIP_TRY(ctx, hist.ensure(static_cast<size_t>(hm) + 8));
      unsigned long long *kin = key_a.p, *kout = key_b.p;
      int32_t *vin = val_a.p, *vout = val_b.p;
      hipStream_t st = ctx->stream;
      LaunchTimer t(ctx, PCP_K_MISC);
      for (int pass = 0; pass < 8; ++pass) {  // 63 key bits: 8 passes of 8 (an even count: the result lands in key_a / val_a)
        const int32_t shift = 8 * pass;
        hipLaunchKernelGGL(k_vr_radix_hist, dim3(static_cast<uint32_t>(blocks)), dim3(kVrBlock), 0, st, kin, voxels, shift, hist.p, blocks);
        PCP_HIP_TRY(ctx, hipMemsetAsync(hist.p + hm, 0, sizeof(int32_t), st));
        PCP_HIP_TRY(ctx, scan_exclusive(st, hist.p, hm + 1, ctx->s_tiles, nullptr));
        hipLaunchKernelGGL(k_vr_radix_scatter, dim3(static_cast<uint32_t>(blocks)), dim3(kVrBlock), 0, st, kin, vin, voxels, shift,
                           hist.p, blocks, kout, vout);
        std::swap(kin, kout);
        std::swap(vin, vout);
      }
      PCP_HIP_TRY(ctx, hipGetLastError());
      const size_t sv = static_cast<size_t>(voxels);
      PCP_HIP_TRY(ctx, vr.out_xyz.ensure(3 * sv + 4));
      PCP_HIP_TRY(ctx, vr.out_rgb.ensure(3 * sv + 16));
      PCP_HIP_TRY(ctx, vr.out_label.ensure(sv + 16));
      PCP_HIP_TRY(ctx, vr.out_count.ensure(sv + 4));
      hipLaunchKernelGGL(k_vr_finish, dim3(static_cast<uint32_t>(blocks)), dim3(kVrBlock), 0, st, voxels, kin, vin, vr_table(ctx), vr.leaf,
                         vr.out_xyz.p, vr.out_rgb.p, vr.out_label.p, vr.out_count.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the sort's scratch is freed at the end of this block)
  }
  vr.voxels = voxels;
  vr.finished = true;
  if (out_voxels) *out_voxels = voxels;
  return PCP_OK;
}

int pcp_voxel_reduce_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, float *out_xyz, uint8_t *out_rgb, uint8_t *out_label,
                           uint32_t *out_count, int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  VoxelReduce &vr = ctx->voxel_reduce;
  if (!vr.live) return set_error(ctx, PCP_ERR_STATE, "pcp_voxel_reduce_fetch: no accumulation (call pcp_voxel_reduce_begin)");
  if (!vr.finished) return set_error(ctx, PCP_ERR_STATE, "pcp_voxel_reduce_fetch: pcp_voxel_reduce_finish has not run");
  if (first < 0 || max_rows < 0) return set_error(ctx, PCP_ERR_INVALID, "pcp_voxel_reduce_fetch: negative first / max_rows");
  if (out_label && !vr.with_label)
    return set_error(ctx, PCP_ERR_STATE, "pcp_voxel_reduce_fetch: out_label asked of an accumulation made without label fusion (pcp_set_label_fusion)");
  const int64_t rows = std::max<int64_t>(0, std::min(max_rows, vr.voxels - first));
  if (out_rows) *out_rows = rows;
  if (rows == 0 || !(out_xyz || out_rgb || out_label || out_count)) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t f = static_cast<size_t>(first), r = static_cast<size_t>(rows);
  if (out_xyz) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_xyz, vr.out_xyz.p + 3 * f, 12 * r, hipMemcpyDeviceToHost, ctx->stream));
  if (out_rgb) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rgb, vr.out_rgb.p + 3 * f, 3 * r, hipMemcpyDeviceToHost, ctx->stream));
  if (out_label) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_label, vr.out_label.p + f, r, hipMemcpyDeviceToHost, ctx->stream));
  if (out_count) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_count, vr.out_count.p + f, 4 * r, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

int pcp_voxel_reduce_stats(pcp_context *ctx, int64_t out[6]) {
  if (!ctx || !out) return PCP_ERR_INVALID;
  const VoxelReduce &vr = ctx->voxel_reduce;
  if (!vr.live) return set_error(ctx, PCP_ERR_STATE, "pcp_voxel_reduce_stats: no accumulation (call pcp_voxel_reduce_begin)");
  out[0] = vr.rows;
  out[1] = vr.finished ? vr.voxels : vr.keyed;
  out[2] = vr.slots;
  out[3] = vr.growths;
  out[4] = vr.partials;
  out[5] = vr.atomics;
  return PCP_OK;
}

int pcp_voxel_reduce_end(pcp_context *ctx) {
  if (!ctx) return PCP_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  vr_drop(ctx);
  return PCP_OK;
}

int pcp_voxel_reduce_host(float leaf, int64_t n, const float *xyz, const uint8_t *rgb, const uint8_t *label, int64_t capacity,
                          float *out_xyz, uint8_t *out_rgb, uint8_t *out_label, uint32_t *out_count, int64_t *out_voxels) {
  if (out_voxels) *out_voxels = 0;
  if (!vg::leaf_ok(leaf)) {
    set_global_error("pcp_voxel_reduce_host: leaf %g outside [1e-4, 1]", static_cast<double>(leaf));
    return PCP_ERR_INVALID;
  }
  if (n < 0 || capacity < 0 || (n > 0 && (!xyz || !rgb)) || (out_label && !label)) {
    set_global_error("pcp_voxel_reduce_host: negative n / capacity, a missing array, or out_label without label");
    return PCP_ERR_INVALID;
  }
  const float inv = vg::inverse_leaf(leaf);
  std::vector<std::pair<uint64_t, int64_t>> order;
  try {
    order.resize(static_cast<size_t>(n));
  } catch (const std::bad_alloc &) {
    set_global_error("pcp_voxel_reduce_host: out of host memory for %lld rows", static_cast<long long>(n));
    return PCP_ERR_NOMEM;
  }
  for (int64_t i = 0; i < n; ++i) {
    int32_t cx, cy, cz;
    const bool ok = vg::cell_of(xyz[3 * i], inv, &cx) & vg::cell_of(xyz[3 * i + 1], inv, &cy) & vg::cell_of(xyz[3 * i + 2], inv, &cz);
    if (!ok) {
      set_global_error("pcp_voxel_reduce_host: row %lld has a non-finite coordinate or lies 2^20 leaves or more from the origin",
                       static_cast<long long>(i));
      return PCP_ERR_RANGE;
    }
    order[static_cast<size_t>(i)] = {vg::key_of(cx, cy, cz), i};
  }
  std::sort(order.begin(), order.end());
  int64_t voxels = 0;
  for (size_t a = 0; a < order.size();) {
    size_t b = a;
    vg::Sums s{{0, 0, 0}, 0u, 0u, 0u, 0u, 0u};
    const uint64_t key = order[a].first;
    int32_t c[3];
    vg::cells_of_key(key, &c[0], &c[1], &c[2]);
    for (; b < order.size() && order[b].first == key; ++b) {
      const int64_t i = order[b].second;
      for (int k = 0; k < 3; ++k) s.q[k] += vg::fixed_of(xyz[3 * i + k]) - vg::corner_of(c[k], leaf);
      s.n += 1u;
      s.r += rgb[3 * i];
      s.g += rgb[3 * i + 1];
      s.b += rgb[3 * i + 2];
      if (label) s.label += label[i];
    }
    if (b - a >= vg::kMaxRowsPerVoxel) {
      set_global_error("pcp_voxel_reduce_host: a voxel holds 2^24 rows or more");
      return PCP_ERR_RANGE;
    }
    if (voxels < capacity) {
      float p[3];
      uint8_t col[3], lab;
      vg::finish_voxel(key, leaf, s, p, col, &lab);
      for (int k = 0; k < 3; ++k) {
        if (out_xyz) out_xyz[3 * voxels + k] = p[k];
        if (out_rgb) out_rgb[3 * voxels + k] = col[k];
      }
      if (out_label) out_label[voxels] = lab;
      if (out_count) out_count[voxels] = s.n;
    }
    voxels += 1;
    a = b;
  }
  if (out_voxels) *out_voxels = voxels;
  return PCP_OK;
}

}  // extern "C"
