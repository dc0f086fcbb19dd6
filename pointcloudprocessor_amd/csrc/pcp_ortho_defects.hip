// pcp_ortho_defects.hip -- surface defects on ortho maps ("Surface defects on ortho maps", SD1-SD9): the depth layer
// of a finished map of either kind (the deviation from the facet's plane, or the radial deviation from the fitted cylinder)
// turned into a signed deviation image against a local reference surface, the pixels beyond a threshold into 8-connected
// regions of one class (hollow / bulge), and every kept region into one row of integers: pixels, measured pixels, sum and
// greatest |deviation|, box, centroid sums, open pixels.  The local reference is the mean of the surface pixels of a square
// window, from two summed-area tables (quanta and surface bits: a row scan and a segmented column scan, prefix sums modulo
// 2^64 as the crack width stage's); the regions come from the crack chain's lock-free union-find on pixel indices (the root
// is the region's first pixel; a tile of 32 x 16 pixels is labelled in LDS first, then the links across tiles), a count per
// root, an exclusive scan over the kept roots in pixel order, and a statistics kernel that merges a wavefront's equal regions
// before its atomics.  The arithmetic is pcp_ortho_defects.hpp's, shared with pcp_ortho_defects_host.  Opt-in: nothing here
// runs unless one of its entry points is called; the map is never modified.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "pcp_internal.hpp"
#include "pcp_crack_map.hpp"
#include "pcp_ortho.hpp"
#include "pcp_ortho_defects.hpp"
#include "pcp_scan.hpp"

namespace pcp {

constexpr int kSdBlock = 256;
constexpr int64_t kSdMaxGrid = 2048;       // workgroups of the grid-stride passes (256 CUs of eight)
constexpr int kSdRowTile = 4 * kSdBlock;   // row scan: four consecutive pixels per lane and round
constexpr int32_t kSdSegmentRows = 64;     // column scan: rows per segment
constexpr int kSdPlanes = 2;               // the tables: quanta, surface bits
// device scalars of a call
enum { SDS_HOLLOW = 0, SDS_BULGE, SDS_UNSUPPORTED, SDS_REFUSED, SDS_FIRST_PASS, SDS_SURFACE, SDS_DROPPED, SDS_SCALARS = 8 };

static inline uint32_t sd_blocks(int64_t n) {
  return static_cast<uint32_t>(std::max<int64_t>(1, std::min<int64_t>(div_up(n, kSdBlock), kSdMaxGrid)));
}
static inline uint32_t sd_blocks_all(int64_t n) { return static_cast<uint32_t>(std::max<int64_t>(1, div_up(n, kSdBlock))); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(v), o, 64));
    v = other > v ? other : v;
  }
  return v;
}

// one atomic per workgroup and count: the wavefronts' sums meet in LDS first (ws: kSdBlock / 64 words; every lane of the
// workgroup calls it).  (One atomic per wavefront: thousands of same-address atomics per counter, a third of a millisecond on
// the probe's map.)
__device__ __forceinline__ void sd_tally(unsigned long long *scalars, int which, uint32_t count, unsigned long long *ws) {
  const unsigned long long all = wave_sum_u64(count);
  if ((threadIdx.x & 63u) == 0u) ws[threadIdx.x >> 6] = all;
  __syncthreads();
  if (threadIdx.x == 0u) {
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < kSdBlock / 64; ++k) sum += ws[k];
    if (sum) atomicAdd(scalars + which, sum);
  }
  __syncthreads();  // (ws is written again by the next count)
}

// SD2 (and SD3b when sat is nullptr: W = 0).  One lane per pixel: the status and the depth through the source image, as
// k_or_layers takes them; the quantum and the flags; with tables to come, their two input planes; without, the class.
__global__ __launch_bounds__(kSdBlock) void k_sd_quantise(int64_t px, const int32_t *__restrict__ source,
                                                          const unsigned long long *__restrict__ keys, sd::Params prm,
                                                          int32_t *__restrict__ qv, uint8_t *__restrict__ flags,
                                                          unsigned long long *__restrict__ sat, int32_t *__restrict__ dev,
                                                          uint8_t *__restrict__ cls, unsigned long long *__restrict__ scalars) {
  __shared__ unsigned long long ws[kSdBlock / 64];
  uint32_t surface = 0u, refused = 0u, hollow = 0u, bulge = 0u;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kSdBlock + threadIdx.x; p < px; p += static_cast<int64_t>(gridDim.x) * kSdBlock) {
    const int32_t src = source[p];
    const uint32_t status = src < 0 ? 0u : (src == p ? 1u : 2u);
    const float depth = src >= 0 ? om::key_depth(keys[src]) : 0.0f;
    int32_t q;
    bool no;
    const bool ok = sd::surface(status, depth, &q, &no);
    surface += ok ? 1u : 0u;
    refused += no ? 1u : 0u;
    qv[p] = q;
    flags[p] = ok ? static_cast<uint8_t>(sd::kSurface | (status == 1u ? sd::kMeasured : 0)) : uint8_t(0);
    if (sat) {
      sat[p] = static_cast<unsigned long long>(static_cast<long long>(q));
      sat[px + p] = ok ? 1ull : 0ull;
    } else {
      const int32_t c = ok ? sd::masked(sd::classify_frame(q, prm.T), prm.classes) : 0;
      dev[p] = q;
      cls[p] = static_cast<uint8_t>(c);
      hollow += c == 1 ? 1u : 0u;
      bulge += c == 2 ? 1u : 0u;
    }
  }
  sd_tally(scalars, SDS_SURFACE, surface, ws);
  sd_tally(scalars, SDS_REFUSED, refused, ws);
  sd_tally(scalars, SDS_HOLLOW, hollow, ws);
  sd_tally(scalars, SDS_BULGE, bulge, ws);
}

// ---- the tables: twins of the crack width stage's three scans, over kSdPlanes planes of w * h --------------------------------
// row scan: one workgroup per (row, plane); the wavefronts' sums meet in LDS, the carry runs along the row
__global__ __launch_bounds__(kSdBlock) void k_sd_rows(unsigned long long *__restrict__ sat, int32_t w, int32_t h) {
  __shared__ unsigned long long ws[kSdBlock / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned long long *row = sat + (static_cast<int64_t>(blockIdx.y) * h + static_cast<int64_t>(blockIdx.x)) * w;
  unsigned long long carry = 0;
  for (int32_t base = 0; base < w; base += kSdRowTile) {
    const int32_t i0 = base + static_cast<int32_t>(threadIdx.x) * 4;
    unsigned long long v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < w ? row[i0 + k] : 0ull;
#pragma unroll
    for (int k = 1; k < 4; ++k) v[k] += v[k - 1];
    const unsigned long long mine = v[3];
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) ws[wid] = incl;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kSdBlock / 64; ++k) {
      if (k < wid) before += ws[k];
      total += ws[k];
    }
    __syncthreads();  // (ws is written again in the next round)
    const unsigned long long off = carry + before + (incl - mine);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < w) row[i0 + k] = off + v[k];
    carry += total;
  }
}

// column scan, segmented: one lane per (column, segment of 64 rows, plane)
__global__ __launch_bounds__(kSdBlock) void k_sd_column_sums(const unsigned long long *__restrict__ sat, int32_t w, int32_t h, int32_t segs,
                                                             unsigned long long *__restrict__ seg) {
  const int32_t x = static_cast<int32_t>(blockIdx.x) * kSdBlock + static_cast<int32_t>(threadIdx.x);
  if (x >= w) return;
  const int32_t s = static_cast<int32_t>(blockIdx.y), a = static_cast<int32_t>(blockIdx.z);
  const unsigned long long *col = sat + static_cast<int64_t>(a) * h * w + x;
  const int32_t y0 = s * kSdSegmentRows, y1 = min(h, y0 + kSdSegmentRows);
  unsigned long long sum = 0;
  for (int32_t y = y0; y < y1; ++y) sum += col[static_cast<int64_t>(y) * w];
  seg[(static_cast<int64_t>(a) * segs + s) * w + x] = sum;
}

__global__ __launch_bounds__(kSdBlock) void k_sd_columns(unsigned long long *__restrict__ sat, int32_t w, int32_t h, int32_t segs,
                                                         const unsigned long long *__restrict__ seg) {
  const int32_t x = static_cast<int32_t>(blockIdx.x) * kSdBlock + static_cast<int32_t>(threadIdx.x);
  if (x >= w) return;
  const int32_t s = static_cast<int32_t>(blockIdx.y), a = static_cast<int32_t>(blockIdx.z);
  const unsigned long long *sg = seg + static_cast<int64_t>(a) * segs * w + x;
  unsigned long long run = 0;
  for (int32_t sp = 0; sp < s; ++sp) run += sg[static_cast<int64_t>(sp) * w];
  unsigned long long *col = sat + static_cast<int64_t>(a) * h * w + x;
  const int32_t y0 = s * kSdSegmentRows, y1 = min(h, y0 + kSdSegmentRows);
  for (int32_t y = y0; y < y1; ++y) {
    run += col[static_cast<int64_t>(y) * w];
    col[static_cast<int64_t>(y) * w] = run;
  }
}

// SD4: the input planes of the second pair of tables: the surface pixels whose first-pass class is 0
__global__ __launch_bounds__(kSdBlock) void k_sd_refill(int64_t px, const int32_t *__restrict__ qv, const uint8_t *__restrict__ flags,
                                                        const uint8_t *__restrict__ cls, unsigned long long *__restrict__ sat) {
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kSdBlock + threadIdx.x; p < px; p += static_cast<int64_t>(gridDim.x) * kSdBlock) {
    const bool in = (flags[p] & sd::kSurface) && cls[p] == 0;
    sat[p] = in ? static_cast<unsigned long long>(static_cast<long long>(qv[p])) : 0ull;
    sat[px + p] = in ? 1ull : 0ull;
  }
}

// SD3 / SD4, one lane per pixel.  kPass 0: the only pass; 1: the first of two (every class bit on, no mask); 2: the second
// (reads the first pass's dev and class, keeps them where its own count misses min_support).
template <int kPass>
__global__ __launch_bounds__(kSdBlock) void k_sd_classify(int64_t px, int32_t w, int32_t h, sd::Params prm, const int32_t *__restrict__ qv,
                                                          uint8_t *__restrict__ flags, const unsigned long long *__restrict__ sat,
                                                          int32_t *__restrict__ dev, uint8_t *__restrict__ cls,
                                                          unsigned long long *__restrict__ scalars) {
  __shared__ unsigned long long ws[kSdBlock / 64];
  uint32_t hollow = 0u, bulge = 0u, unsupported = 0u, first = 0u;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kSdBlock + threadIdx.x; p < px; p += static_cast<int64_t>(gridDim.x) * kSdBlock) {
    const uint8_t f = flags[p];
    if (!(f & sd::kSurface)) {
      if constexpr (kPass != 2) {
        dev[p] = 0;
        cls[p] = 0;
      }
      continue;
    }
    const int32_t r = static_cast<int32_t>(p / w), c = static_cast<int32_t>(p - static_cast<int64_t>(r) * w);
    int64_t S, n;
    sd::window(sat, sat + px, w, h, r, c, prm.W, &S, &n);
    int32_t d = 0, k = 0;
    if (n >= prm.min_support) {
      k = sd::classify(qv[p], S, n, prm.T, &d);
    } else if constexpr (kPass == 2) {
      d = dev[p];
      k = cls[p];
      flags[p] = static_cast<uint8_t>(f | sd::kFirstPass);
      first += 1u;
    } else {
      unsupported += 1u;
    }
    if constexpr (kPass != 1) {
      k = sd::masked(k, prm.classes);
      hollow += k == 1 ? 1u : 0u;
      bulge += k == 2 ? 1u : 0u;
    }
    dev[p] = d;
    cls[p] = static_cast<uint8_t>(k);
  }
  sd_tally(scalars, SDS_HOLLOW, hollow, ws);
  sd_tally(scalars, SDS_BULGE, bulge, ws);
  sd_tally(scalars, SDS_UNSUPPORTED, unsupported, ws);
  sd_tally(scalars, SDS_FIRST_PASS, first, ws);
}

// ---- SD5: the regions ------------------------------------------------------------------------------------------------------
// the links of pixel (r, c) of class k that SD5 needs: W, and N -- or, where N is not of the class, NW and NE (where N is of the
// class, NW and NE need no link of their own: each of them is N's W or E neighbour and linked with it by that pixel's W
// link).  visit(dr, dc) for each.
template <typename Visit>
__device__ __forceinline__ void sd_links(const uint8_t *__restrict__ cls, int64_t p, int32_t w, int32_t r, int32_t c, uint8_t k, Visit visit) {
  if (c > 0 && cls[p - 1] == k) visit(0, -1);
  if (r > 0) {
    if (cls[p - w] == k) {
      visit(-1, 0);
    } else {
      if (c > 0 && cls[p - w - 1] == k) visit(-1, -1);
      if (c < w - 1 && cls[p - w + 1] == k) visit(-1, 1);
    }
  }
}

// the tiled form: a workgroup labels a tile of 32 x 16 pixels in LDS first (parents as tile-local indices: the order of the
// local indices is the order of the pixels, so a local root is the tile's first pixel of its region), then writes the global
// parents; k_sd_tile_borders unites the links that leave a tile: from its top row, its left and its right column.
constexpr int kSdTileW = 32, kSdTileH = 16, kSdTile = kSdTileW * kSdTileH;

__device__ __forceinline__ int32_t sd_local_find(const volatile int32_t *par, int32_t v) {
  for (int32_t p = par[v]; p != v; p = par[v]) v = p;  // (p < v)
  return v;
}

// cc_unite's rule on the tile's words: the larger root is hooked under the smaller one by compare-and-swap; a failed swap
// means the larger root has been hooked meanwhile, so max(a, b) strictly decreases.  No lane waits for another one.
__device__ __forceinline__ void sd_local_unite(int32_t *par, int32_t a, int32_t b) {
  for (;;) {
    a = sd_local_find(par, a);
    b = sd_local_find(par, b);
    if (a == b) return;
    const int32_t hi = max(a, b), lo = min(a, b);
    if (atomicCAS(par + hi, hi, lo) == hi) return;
    a = hi;
    b = lo;
  }
}

__global__ __launch_bounds__(kSdTile) void k_sd_tile_label(int32_t w, int32_t h, const uint8_t *__restrict__ cls, int32_t *__restrict__ parent) {
  __shared__ int32_t par[kSdTile];
  const int32_t lx = static_cast<int32_t>(threadIdx.x), ly = static_cast<int32_t>(threadIdx.y), l = ly * kSdTileW + lx;
  const int32_t c = static_cast<int32_t>(blockIdx.x) * kSdTileW + lx, r = static_cast<int32_t>(blockIdx.y) * kSdTileH + ly;
  const bool inside = c < w && r < h;
  const int64_t p = static_cast<int64_t>(r) * w + c;
  const uint8_t k = inside ? cls[p] : uint8_t(0);
  par[l] = l;
  __syncthreads();
  if (k)
    sd_links(cls, p, w, r, c, k, [&](int32_t dr, int32_t dc) {
      if (ly + dr >= 0 && lx + dc >= 0 && lx + dc < kSdTileW) sd_local_unite(par, l, l + dr * kSdTileW + dc);
    });
  __syncthreads();
  if (!inside) return;
  const int32_t root = k ? sd_local_find(par, l) : l;
  const int32_t r0 = static_cast<int32_t>(blockIdx.y) * kSdTileH + root / kSdTileW, c0 = static_cast<int32_t>(blockIdx.x) * kSdTileW + root % kSdTileW;
  parent[p] = r0 * w + c0;
}

// the links that leave the tile, one lane per pixel of a tile's top row, left column or right column
__global__ __launch_bounds__(kSdBlock) void k_sd_tile_borders(int64_t px, int32_t w, const uint8_t *__restrict__ cls, int32_t *parent) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kSdBlock + threadIdx.x;
  if (p >= px) return;
  const int32_t r = static_cast<int32_t>(p / w), c = static_cast<int32_t>(p - static_cast<int64_t>(r) * w);
  const int32_t lx = c % kSdTileW, ly = r % kSdTileH;
  if (ly != 0 && lx != 0 && lx != kSdTileW - 1) return;
  const uint8_t k = cls[p];
  if (!k) return;
  const int32_t me = static_cast<int32_t>(p);
  sd_links(cls, p, w, r, c, k, [&](int32_t dr, int32_t dc) {
    if (!(ly + dr >= 0 && lx + dc >= 0 && lx + dc < kSdTileW)) cc_unite(parent, me, me + dr * w + dc);
  });
}

// after the union kernel has ended the forest is final: the root of every classed pixel (-1: not classed), and the pixels per
// root (a wavefront's lanes are neighbours in a row and mostly of one region: one atomic then)
__global__ __launch_bounds__(kSdBlock) void k_sd_flatten(int64_t px, const uint8_t *__restrict__ cls, const int32_t *__restrict__ parent,
                                                         int32_t *__restrict__ root_of, int32_t *__restrict__ size) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kSdBlock + threadIdx.x;
  const bool valid = p < px && cls[p] != 0;
  int32_t v = -1;
  if (valid) {
    v = static_cast<int32_t>(p);
    for (int32_t q = parent[v]; q != v; q = parent[v]) v = q;  // (q < v)
  }
  if (p < px) root_of[p] = v;
  bool shared;
  const bool issue = wave_row_issuer(valid, v, &shared);
  const int32_t count = shared ? static_cast<int32_t>(__popcll(__ballot(valid))) : 1;
  if (issue) atomicAdd(size + v, count);
}

// the flag the scan counts: pixel p is the root of a kept region; [px] = 0 (the scan's total goes there).  Counts the dropped.
__global__ __launch_bounds__(kSdBlock) void k_sd_keep(int64_t px, const int32_t *__restrict__ root_of, const int32_t *__restrict__ size,
                                                      int32_t min_pixels, int32_t *__restrict__ rank,
                                                      unsigned long long *__restrict__ scalars) {
  __shared__ unsigned long long ws[kSdBlock / 64];
  uint32_t dropped = 0u;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kSdBlock + threadIdx.x; p <= px; p += static_cast<int64_t>(gridDim.x) * kSdBlock) {
    int32_t flag = 0;
    if (p < px && root_of[p] == static_cast<int32_t>(p)) {
      flag = size[p] >= min_pixels ? 1 : 0;
      dropped += flag ? 0u : 1u;
    }
    rank[p] = flag;
  }
  sd_tally(scalars, SDS_DROPPED, dropped, ws);
}

__global__ __launch_bounds__(kSdBlock) void k_sd_table_init(int64_t rows, unsigned long long *__restrict__ table) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kSdBlock + threadIdx.x;
  if (i >= rows * sd::kRowWords) return;
  const int col = static_cast<int>(i % sd::kRowWords);
  table[i] = (col == sd::R_COL_MIN || col == sd::R_ROW_MIN) ? ~0ull : 0ull;
}

// SD7, one lane per pixel: the region id of the pixel and its share of the region's row.  Where all the live lanes of a
// wavefront share a region their values are merged first and one lane issues the atomics.  Column R_MAX holds the word of
// sd::best_word until k_sd_table_final splits it.
__global__ __launch_bounds__(kSdBlock) void k_sd_stats(int64_t px, int32_t w, int32_t h, int32_t min_pixels, const uint8_t *__restrict__ cls,
                                                       const uint8_t *__restrict__ flags, const int32_t *__restrict__ dev,
                                                       const int32_t *__restrict__ root_of, const int32_t *__restrict__ size,
                                                       const int32_t *__restrict__ rank, int32_t *__restrict__ region,
                                                       unsigned long long *__restrict__ table) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kSdBlock + threadIdx.x;
  bool valid = false;
  int32_t row = -1;
  unsigned long long pixels = 0, measured = 0, sum = 0, best = 0, sum_col = 0, sum_row = 0, open = 0, first = 0;
  uint32_t c_lo = 0xffffffffu, c_hi = 0u, r_lo = 0xffffffffu, r_hi = 0u;
  if (p < px) {
    const int32_t root = root_of[p];
    if (root >= 0 && size[root] >= min_pixels) {
      valid = true;
      row = rank[root];
      const int32_t r = static_cast<int32_t>(p / w), c = static_cast<int32_t>(p - static_cast<int64_t>(r) * w);
      const uint8_t f = flags[p];
      const int32_t d = dev[p];
      pixels = 1;
      measured = (f & sd::kMeasured) ? 1 : 0;
      best = sd::best_word(d, p);
      sum = static_cast<unsigned long long>(sd::best_abs(best));
      c_lo = c_hi = static_cast<uint32_t>(c);
      r_lo = r_hi = static_cast<uint32_t>(r);
      sum_col = static_cast<unsigned long long>(c);
      sum_row = static_cast<unsigned long long>(r);
      open = sd::open_pixel(flags, w, h, r, c) ? 1 : 0;
      first = (f & sd::kFirstPass) ? 1 : 0;
      if (root == static_cast<int32_t>(p)) {  // the region's first pixel: the two columns no other lane writes
        table[static_cast<int64_t>(sd::kRowWords) * row + sd::R_CLASS] = cls[p];
        table[static_cast<int64_t>(sd::kRowWords) * row + sd::R_FIRST] = static_cast<unsigned long long>(p);
      }
    }
    region[p] = valid ? row + 1 : 0;
  }
  bool shared;
  const bool issue = wave_row_issuer(valid, row, &shared);
  if (shared) {
    pixels = wave_sum_u64(pixels);
    measured = wave_sum_u64(measured);
    sum = wave_sum_u64(sum);
    best = wave_max_u64(best);
    sum_col = wave_sum_u64(sum_col);
    sum_row = wave_sum_u64(sum_row);
    open = wave_sum_u64(open);
    first = wave_sum_u64(first);
    c_lo = wave_min_u32(c_lo);
    c_hi = wave_max_u32(c_hi);
    r_lo = wave_min_u32(r_lo);
    r_hi = wave_max_u32(r_hi);
  }
  if (!issue) return;
  unsigned long long *t = table + static_cast<int64_t>(sd::kRowWords) * row;
  atomicAdd(t + sd::R_PIXELS, pixels);
  if (measured) atomicAdd(t + sd::R_MEASURED, measured);
  atomicAdd(t + sd::R_SUM, sum);
  atomicMax(t + sd::R_MAX, best);
  atomicMin(t + sd::R_COL_MIN, static_cast<unsigned long long>(c_lo));
  atomicMax(t + sd::R_COL_MAX, static_cast<unsigned long long>(c_hi));
  atomicMin(t + sd::R_ROW_MIN, static_cast<unsigned long long>(r_lo));
  atomicMax(t + sd::R_ROW_MAX, static_cast<unsigned long long>(r_hi));
  atomicAdd(t + sd::R_SUM_COL, sum_col);
  atomicAdd(t + sd::R_SUM_ROW, sum_row);
  if (open) atomicAdd(t + sd::R_OPEN, open);
  if (first) atomicAdd(t + sd::R_FIRST_PASS, first);
}

__global__ __launch_bounds__(kSdBlock) void k_sd_table_final(int64_t rows, unsigned long long *__restrict__ table) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kSdBlock + threadIdx.x;
  if (i >= rows) return;
  unsigned long long *t = table + static_cast<int64_t>(sd::kRowWords) * i;
  const unsigned long long best = t[sd::R_MAX];
  t[sd::R_MAX] = static_cast<unsigned long long>(sd::best_abs(best));
  t[sd::R_MAX_PIXEL] = static_cast<unsigned long long>(sd::best_pixel(best));
}

hipError_t preload_ortho_defects() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_sd_stats));
}

// SD1: the message of a refusal into msg; PCP_OK fills *out
static int sd_check(const char *who, const pcp_ortho_defect_params *p, sd::Params *out, char *msg, size_t cap) {
  const char *bad = sd::bad_field(p->threshold, p->window_px, p->refine, p->min_support, p->min_pixels, p->classes);
  if (bad) {
    if (!std::strcmp(bad, "threshold"))
      std::snprintf(msg, cap, "%s: threshold %g outside [2^-20, 1] metres", who, static_cast<double>(p->threshold));
    else if (!std::strcmp(bad, "window_px"))
      std::snprintf(msg, cap, "%s: window_px %d outside 0..%d", who, p->window_px, sd::kMaxWindow);
    else if (!std::strcmp(bad, "refine"))
      std::snprintf(msg, cap, "%s: refine %d: 0 or 1, and 1 needs window_px > 0 (it is %d)", who, p->refine, p->window_px);
    else if (!std::strcmp(bad, "min_support"))
      std::snprintf(msg, cap, "%s: min_support %d below 1", who, p->min_support);
    else if (!std::strcmp(bad, "min_pixels"))
      std::snprintf(msg, cap, "%s: min_pixels %d below 1", who, p->min_pixels);
    else
      std::snprintf(msg, cap, "%s: classes %d: bit 0 hollows, bit 1 bulges, not 0", who, p->classes);
    return PCP_ERR_INVALID;
  }
  out->T = sd::quanta_of(p->threshold);
  out->W = p->window_px;
  out->refine = p->refine;
  out->min_support = p->window_px > 0 ? p->min_support : 1;
  out->min_pixels = p->min_pixels;
  out->classes = p->classes;
  return PCP_OK;
}

// the tables of the two planes in sat (w * h each), in place
static int sd_tables(pcp_context *ctx, unsigned long long *sat, unsigned long long *seg, int32_t w, int32_t h, int32_t segs) {
  LaunchTimer t(ctx, PCP_K_MISC);
  const uint32_t xb = static_cast<uint32_t>((w + kSdBlock - 1) / kSdBlock);
  hipLaunchKernelGGL(k_sd_rows, dim3(static_cast<uint32_t>(h), kSdPlanes), dim3(kSdBlock), 0, ctx->stream, sat, w, h);
  hipLaunchKernelGGL(k_sd_column_sums, dim3(xb, static_cast<uint32_t>(segs), kSdPlanes), dim3(kSdBlock), 0, ctx->stream, sat, w, h, segs, seg);
  hipLaunchKernelGGL(k_sd_columns, dim3(xb, static_cast<uint32_t>(segs), kSdPlanes), dim3(kSdBlock), 0, ctx->stream, sat, w, h, segs, seg);
  PCP_HIP_TRY(ctx, hipGetLastError());
  return PCP_OK;
}

static int sd_run(pcp_context *ctx, const sd::Params &prm, int64_t out[8]) {
  const OrthoMap &m = ctx->ortho;
  OrthoDefects &d = ctx->ortho_defects;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int32_t w = m.frame.width, h = m.frame.height;
  const int64_t px = static_cast<int64_t>(w) * h;
  const size_t spx = static_cast<size_t>(px);
  const int32_t segs = (h + kSdSegmentRows - 1) / kSdSegmentRows;
  d.live = false;
  d.rows = 0;
  PCP_HIP_TRY(ctx, d.dev.ensure(spx + 4));
  PCP_HIP_TRY(ctx, d.region.ensure(spx + 4));
  PCP_HIP_TRY(ctx, d.cls.ensure(spx + 16));
  // the scratch of a call is its own and goes when it returns
  DevBuf<int32_t> qv, parent, root_of, size, rank, tiles;
  DevBuf<uint8_t> flags;
  DevBuf<unsigned long long> sat, seg, scalars;
  PCP_HIP_TRY(ctx, qv.ensure(spx + 4));
  PCP_HIP_TRY(ctx, flags.ensure(spx + 16));
  PCP_HIP_TRY(ctx, scalars.ensure(SDS_SCALARS));
  PCP_HIP_TRY(ctx, hipMemsetAsync(scalars.p, 0, SDS_SCALARS * 8, ctx->stream));
  if (prm.W > 0) {
    PCP_HIP_TRY(ctx, sat.ensure(kSdPlanes * spx + 4));
    PCP_HIP_TRY(ctx, seg.ensure(static_cast<size_t>(kSdPlanes) * segs * w + 4));
  }
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_sd_quantise, dim3(sd_blocks(px)), dim3(kSdBlock), 0, ctx->stream, px, m.source.p, m.keys.p, prm, qv.p, flags.p, sat.p,
                       d.dev.p, d.cls.p, scalars.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  if (prm.W > 0) {
    int rc = sd_tables(ctx, sat.p, seg.p, w, h, segs);
    if (rc != PCP_OK) return rc;
    {
      LaunchTimer t(ctx, PCP_K_MISC);
      if (prm.refine)
        hipLaunchKernelGGL(k_sd_classify<1>, dim3(sd_blocks(px)), dim3(kSdBlock), 0, ctx->stream, px, w, h, prm, qv.p, flags.p, sat.p, d.dev.p,
                           d.cls.p, scalars.p);
      else
        hipLaunchKernelGGL(k_sd_classify<0>, dim3(sd_blocks(px)), dim3(kSdBlock), 0, ctx->stream, px, w, h, prm, qv.p, flags.p, sat.p, d.dev.p,
                           d.cls.p, scalars.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    if (prm.refine) {
      {
        LaunchTimer t(ctx, PCP_K_MISC);
        hipLaunchKernelGGL(k_sd_refill, dim3(sd_blocks(px)), dim3(kSdBlock), 0, ctx->stream, px, qv.p, flags.p, d.cls.p, sat.p);
        PCP_HIP_TRY(ctx, hipGetLastError());
      }
      rc = sd_tables(ctx, sat.p, seg.p, w, h, segs);
      if (rc != PCP_OK) return rc;
      LaunchTimer t(ctx, PCP_K_MISC);
      hipLaunchKernelGGL(k_sd_classify<2>, dim3(sd_blocks(px)), dim3(kSdBlock), 0, ctx->stream, px, w, h, prm, qv.p, flags.p, sat.p, d.dev.p,
                         d.cls.p, scalars.p);
      PCP_HIP_TRY(ctx, hipGetLastError());
    }
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    sat.release();  // (the labelling's scratch takes its place)
    seg.release();
  }
  // SD5
  PCP_HIP_TRY(ctx, parent.ensure(spx + 4));
  PCP_HIP_TRY(ctx, root_of.ensure(spx + 4));
  PCP_HIP_TRY(ctx, size.ensure(spx + 4));
  PCP_HIP_TRY(ctx, rank.ensure(spx + 8));
  PCP_HIP_TRY(ctx, hipMemsetAsync(size.p, 0, spx * 4, ctx->stream));
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_sd_tile_label, dim3(static_cast<uint32_t>(div_up(w, kSdTileW)), static_cast<uint32_t>(div_up(h, kSdTileH))),
                       dim3(kSdTileW, kSdTileH), 0, ctx->stream, w, h, d.cls.p, parent.p);
    hipLaunchKernelGGL(k_sd_tile_borders, dim3(sd_blocks_all(px)), dim3(kSdBlock), 0, ctx->stream, px, w, d.cls.p, parent.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    hipLaunchKernelGGL(k_sd_flatten, dim3(sd_blocks_all(px)), dim3(kSdBlock), 0, ctx->stream, px, d.cls.p, parent.p, root_of.p, size.p);
    hipLaunchKernelGGL(k_sd_keep, dim3(sd_blocks(px + 1)), dim3(kSdBlock), 0, ctx->stream, px, root_of.p, size.p, prm.min_pixels, rank.p, scalars.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
    PCP_HIP_TRY(ctx, scan_exclusive(ctx->stream, rank.p, px + 1, tiles, nullptr));  // [px] = the number of kept regions
  }
  int32_t kept = 0;
  unsigned long long hs[SDS_SCALARS];
  PCP_HIP_TRY(ctx, hipMemcpyAsync(&kept, rank.p + px, 4, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipMemcpyAsync(hs, scalars.p, sizeof hs, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (kept < 0 || kept > px) return set_error(ctx, PCP_ERR_DEVICE, "pcp_ortho_defects: %d regions for %lld pixels", kept, static_cast<long long>(px));
  const int64_t rows = kept;
  PCP_HIP_TRY(ctx, d.table.ensure(static_cast<size_t>(sd::kRowWords) * static_cast<size_t>(rows) + 4));
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    if (rows > 0)
      hipLaunchKernelGGL(k_sd_table_init, dim3(sd_blocks_all(rows * sd::kRowWords)), dim3(kSdBlock), 0, ctx->stream, rows, d.table.p);
    hipLaunchKernelGGL(k_sd_stats, dim3(sd_blocks_all(px)), dim3(kSdBlock), 0, ctx->stream, px, w, h, prm.min_pixels, d.cls.p, flags.p, d.dev.p,
                       root_of.p, size.p, rank.p, d.region.p, d.table.p);
    if (rows > 0) hipLaunchKernelGGL(k_sd_table_final, dim3(sd_blocks_all(rows)), dim3(kSdBlock), 0, ctx->stream, rows, d.table.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the scratch is freed on return)
  d.out[sd::O_KEPT] = rows;
  d.out[sd::O_DROPPED] = static_cast<int64_t>(hs[SDS_DROPPED]);
  d.out[sd::O_HOLLOW] = static_cast<int64_t>(hs[SDS_HOLLOW]);
  d.out[sd::O_BULGE] = static_cast<int64_t>(hs[SDS_BULGE]);
  d.out[sd::O_UNSUPPORTED] = static_cast<int64_t>(hs[SDS_UNSUPPORTED]);
  d.out[sd::O_REFUSED] = static_cast<int64_t>(hs[SDS_REFUSED]);
  d.out[sd::O_FIRST_PASS] = static_cast<int64_t>(hs[SDS_FIRST_PASS]);
  d.out[sd::O_SURFACE] = static_cast<int64_t>(hs[SDS_SURFACE]);
  d.rows = rows;
  d.live = true;
  for (int k = 0; k < sd::kOutWords; ++k) out[k] = d.out[k];
  return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_ortho_defects(pcp_context *ctx, const pcp_ortho_defect_params *params, int64_t out[8]) {
  if (!ctx) return PCP_ERR_INVALID;
  if (!params) return set_error(ctx, PCP_ERR_INVALID, "pcp_ortho_defects: NULL params");
  if (!out) return set_error(ctx, PCP_ERR_INVALID, "pcp_ortho_defects: NULL out");
  sd::Params prm;
  char msg[256];
  if (sd_check("pcp_ortho_defects", params, &prm, msg, sizeof msg) != PCP_OK) return set_error(ctx, PCP_ERR_INVALID, "%s", msg);
  const OrthoMap &m = ctx->ortho;
  if (!m.live) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_defects: no map (call pcp_ortho_begin or pcp_ortho_begin_cyl)");
  if (!m.finished) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_defects: pcp_ortho_finish has not run");
  return sd_run(ctx, prm, out);
}

int pcp_ortho_defects_fetch(pcp_context *ctx, int32_t *out_dev, uint8_t *out_class, int32_t *out_region) {
  if (!ctx) return PCP_ERR_INVALID;
  const OrthoDefects &d = ctx->ortho_defects;
  if (!d.live || !ctx->ortho.live) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_defects_fetch: no results (pcp_ortho_defects on the finished map)");
  if (!(out_dev || out_class || out_region)) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t px = static_cast<size_t>(ctx->ortho.frame.width) * static_cast<size_t>(ctx->ortho.frame.height);
  if (out_dev) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_dev, d.dev.p, 4 * px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_class) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_class, d.cls.p, px, hipMemcpyDeviceToHost, ctx->stream));
  if (out_region) PCP_HIP_TRY(ctx, hipMemcpyAsync(out_region, d.region.p, 4 * px, hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PCP_OK;
}

int pcp_ortho_defects_table(pcp_context *ctx, int64_t first, int64_t max_rows, int64_t *out_rows16, int64_t *out_rows) {
  if (!ctx) return PCP_ERR_INVALID;
  if (out_rows) *out_rows = 0;
  if (first < 0 || max_rows < 0) return set_error(ctx, PCP_ERR_INVALID, "pcp_ortho_defects_table: negative first or max_rows");
  const OrthoDefects &d = ctx->ortho_defects;
  if (!d.live || !ctx->ortho.live) return set_error(ctx, PCP_ERR_STATE, "pcp_ortho_defects_table: no results (pcp_ortho_defects on the finished map)");
  const int64_t rows = std::max<int64_t>(0, std::min(max_rows, d.rows - first));
  if (rows == 0) return PCP_OK;
  if (out_rows16) {
    PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
    PCP_HIP_TRY(ctx, hipMemcpyAsync(out_rows16, d.table.p + sd::kRowWords * static_cast<size_t>(first), sd::kRowWords * static_cast<size_t>(rows) * 8,
                                    hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

// SD9: the same header, sequential tables, a sequential labelling with the same roots, the same tie rules
int pcp_ortho_defects_host(int32_t width, int32_t height, const float *depth, const uint8_t *status, const pcp_ortho_defect_params *params,
                           int64_t out[8], int32_t *out_dev, uint8_t *out_class, int32_t *out_region, int64_t *out_rows16, int64_t max_rows,
                           int64_t *out_rows) {
  const char *who = "pcp_ortho_defects_host";
  if (out_rows) *out_rows = 0;
  if (!params || !out || !depth || !status) {
    set_global_error("%s: NULL params, out, depth or status", who);
    return PCP_ERR_INVALID;
  }
  sd::Params prm;
  char msg[256];
  if (sd_check(who, params, &prm, msg, sizeof msg) != PCP_OK) {
    set_global_error("%s", msg);
    return PCP_ERR_INVALID;
  }
  if (width < 1 || height < 1 || width > om::kMaxSide || height > om::kMaxSide || static_cast<int64_t>(width) * height > om::kMaxPixels) {
    set_global_error("%s: width %d, height %d outside 1..16384 a side and 2^26 pixels", who, width, height);
    return PCP_ERR_INVALID;
  }
  if (max_rows < 0) {
    set_global_error("%s: negative max_rows", who);
    return PCP_ERR_INVALID;
  }
  const int32_t w = width, h = height;
  const int64_t px = static_cast<int64_t>(w) * h;
  const size_t spx = static_cast<size_t>(px);
  std::vector<int32_t> qv, dev, parent, size, rank;
  std::vector<uint8_t> flags, cls;
  std::vector<unsigned long long> sat;
  try {
    qv.assign(spx, 0);
    dev.assign(spx, 0);
    parent.resize(spx);
    size.assign(spx, 0);
    rank.assign(spx, -1);
    flags.assign(spx, 0);
    cls.assign(spx, 0);
    if (prm.W > 0) sat.resize(2 * spx);
  } catch (const std::bad_alloc &) {
    set_global_error("%s: out of host memory for %d x %d pixels", who, w, h);
    return PCP_ERR_NOMEM;
  }
  for (int k = 0; k < sd::kOutWords; ++k) out[k] = 0;
  for (size_t p = 0; p < spx; ++p) {  // SD2
    bool no;
    const bool ok = sd::surface(status[p], depth[p], &qv[p], &no);
    flags[p] = ok ? static_cast<uint8_t>(sd::kSurface | (status[p] == 1 ? sd::kMeasured : 0)) : uint8_t(0);
    out[sd::O_SURFACE] += ok ? 1 : 0;
    out[sd::O_REFUSED] += no ? 1 : 0;
  }
  auto tables = [&](bool second) {  // SD3 / SD4: inclusive prefix sums modulo 2^64, rows then columns
    for (size_t p = 0; p < spx; ++p) {
      const bool in = (flags[p] & sd::kSurface) && (!second || cls[p] == 0);
      sat[p] = in ? static_cast<unsigned long long>(static_cast<long long>(qv[p])) : 0ull;
      sat[spx + p] = in ? 1ull : 0ull;
    }
    for (int a = 0; a < 2; ++a) {
      unsigned long long *t = sat.data() + a * spx;
      for (int32_t r = 0; r < h; ++r)
        for (int32_t c = 1; c < w; ++c) t[static_cast<size_t>(r) * w + c] += t[static_cast<size_t>(r) * w + c - 1];
      for (int32_t r = 1; r < h; ++r)
        for (int32_t c = 0; c < w; ++c) t[static_cast<size_t>(r) * w + c] += t[static_cast<size_t>(r - 1) * w + c];
    }
  };
  if (prm.W == 0) {  // SD3b
    for (size_t p = 0; p < spx; ++p) {
      dev[p] = qv[p];
      cls[p] = (flags[p] & sd::kSurface) ? static_cast<uint8_t>(sd::classify_frame(qv[p], prm.T)) : uint8_t(0);
    }
  } else {
    for (int pass = 0; pass <= prm.refine; ++pass) {
      tables(pass == 1);
      for (int32_t r = 0; r < h; ++r)
        for (int32_t c = 0; c < w; ++c) {
          const size_t p = static_cast<size_t>(r) * w + c;
          if (!(flags[p] & sd::kSurface)) continue;
          int64_t S, n;
          sd::window(sat.data(), sat.data() + spx, w, h, r, c, prm.W, &S, &n);
          if (n >= prm.min_support) {
            cls[p] = static_cast<uint8_t>(sd::classify(qv[p], S, n, prm.T, &dev[p]));
          } else if (pass == 1) {
            flags[p] = static_cast<uint8_t>(flags[p] | sd::kFirstPass);
            out[sd::O_FIRST_PASS] += 1;
          } else {
            out[sd::O_UNSUPPORTED] += 1;
          }
        }
    }
  }
  for (size_t p = 0; p < spx; ++p) {  // the mask, after the last pass only
    cls[p] = static_cast<uint8_t>(sd::masked(cls[p], prm.classes));
    out[sd::O_HOLLOW] += cls[p] == 1 ? 1 : 0;
    out[sd::O_BULGE] += cls[p] == 2 ? 1 : 0;
  }
  // SD5: a sequential union-find whose roots are the lowest indices
  auto find = [&](int32_t v) {
    int32_t root = v;
    while (parent[static_cast<size_t>(root)] != root) root = parent[static_cast<size_t>(root)];
    while (parent[static_cast<size_t>(v)] != root) {
      const int32_t next = parent[static_cast<size_t>(v)];
      parent[static_cast<size_t>(v)] = root;
      v = next;
    }
    return root;
  };
  auto unite = [&](int32_t a, int32_t b) {
    a = find(a);
    b = find(b);
    if (a != b) parent[static_cast<size_t>(std::max(a, b))] = std::min(a, b);
  };
  for (size_t p = 0; p < spx; ++p) parent[p] = static_cast<int32_t>(p);
  for (int32_t r = 0; r < h; ++r)
    for (int32_t c = 0; c < w; ++c) {
      const int32_t p = r * w + c;
      const uint8_t k = cls[static_cast<size_t>(p)];
      if (!k) continue;
      if (c > 0 && cls[static_cast<size_t>(p - 1)] == k) unite(p, p - 1);
      if (r > 0) {
        if (c > 0 && cls[static_cast<size_t>(p - w - 1)] == k) unite(p, p - w - 1);
        if (cls[static_cast<size_t>(p - w)] == k) unite(p, p - w);
        if (c < w - 1 && cls[static_cast<size_t>(p - w + 1)] == k) unite(p, p - w + 1);
      }
    }
  for (size_t p = 0; p < spx; ++p)
    if (cls[p]) size[static_cast<size_t>(find(static_cast<int32_t>(p)))] += 1;
  int64_t rows = 0;
  for (size_t p = 0; p < spx; ++p)  // ids in ascending order of the first pixel
    if (cls[p] && parent[p] == static_cast<int32_t>(p)) {
      if (size[p] >= prm.min_pixels)
        rank[p] = static_cast<int32_t>(rows++);
      else
        out[sd::O_DROPPED] += 1;
    }
  out[sd::O_KEPT] = rows;
  std::vector<int64_t> table;
  try {
    table.assign(static_cast<size_t>(rows) * sd::kRowWords, 0);
  } catch (const std::bad_alloc &) {
    set_global_error("%s: out of host memory for %lld rows", who, static_cast<long long>(rows));
    return PCP_ERR_NOMEM;
  }
  std::vector<uint64_t> best(static_cast<size_t>(rows), 0);
  for (int32_t r = 0; r < h; ++r)
    for (int32_t c = 0; c < w; ++c) {
      const size_t p = static_cast<size_t>(r) * w + c;
      const int32_t row = cls[p] ? rank[static_cast<size_t>(find(static_cast<int32_t>(p)))] : -1;
      if (out_region) out_region[p] = row + 1;
      if (row < 0) continue;
      int64_t *t = table.data() + static_cast<size_t>(row) * sd::kRowWords;
      if (t[sd::R_PIXELS] == 0) {  // the region's first pixel
        t[sd::R_CLASS] = cls[p];
        t[sd::R_FIRST] = static_cast<int64_t>(p);
        t[sd::R_COL_MIN] = t[sd::R_COL_MAX] = c;
        t[sd::R_ROW_MIN] = t[sd::R_ROW_MAX] = r;
      }
      const uint64_t word = sd::best_word(dev[p], static_cast<int64_t>(p));
      best[static_cast<size_t>(row)] = std::max(best[static_cast<size_t>(row)], word);
      t[sd::R_PIXELS] += 1;
      t[sd::R_MEASURED] += (flags[p] & sd::kMeasured) ? 1 : 0;
      t[sd::R_SUM] += sd::best_abs(word);
      t[sd::R_COL_MIN] = std::min<int64_t>(t[sd::R_COL_MIN], c);
      t[sd::R_COL_MAX] = std::max<int64_t>(t[sd::R_COL_MAX], c);
      t[sd::R_ROW_MIN] = std::min<int64_t>(t[sd::R_ROW_MIN], r);
      t[sd::R_ROW_MAX] = std::max<int64_t>(t[sd::R_ROW_MAX], r);
      t[sd::R_SUM_COL] += c;
      t[sd::R_SUM_ROW] += r;
      t[sd::R_OPEN] += sd::open_pixel(flags.data(), w, h, r, c) ? 1 : 0;
      t[sd::R_FIRST_PASS] += (flags[p] & sd::kFirstPass) ? 1 : 0;
    }
  for (int64_t i = 0; i < rows; ++i) {
    table[static_cast<size_t>(i) * sd::kRowWords + sd::R_MAX] = sd::best_abs(best[static_cast<size_t>(i)]);
    table[static_cast<size_t>(i) * sd::kRowWords + sd::R_MAX_PIXEL] = sd::best_pixel(best[static_cast<size_t>(i)]);
  }
  if (out_dev) std::copy(dev.begin(), dev.end(), out_dev);
  if (out_class) std::copy(cls.begin(), cls.end(), out_class);
  if (out_rows16) std::copy(table.begin(), table.begin() + static_cast<std::ptrdiff_t>(std::min(rows, max_rows) * sd::kRowWords), out_rows16);
  if (out_rows) *out_rows = rows;
  return PCP_OK;
}

}  // extern "C"
