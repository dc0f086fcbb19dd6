// pcp_internal.hpp -- context, device parameter blocks and launch/timing helpers
// shared by the translation units of libpcp_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "pcp_hip.h"
#include "pcp_register.hpp"

namespace pcp {

// ---- device-side parameter blocks (passed by value as kernel arguments, so they
// land in SGPRs through the kernarg segment; nothing here is per-lane) ----------
struct DevCamera {
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
  double slack;  // 0.05, view_culling.cpp:157
  float ds_f;    // 14.0f
  double img_wd, img_hd;  // image size as fp64 / cull size as fp32: bounds of the truncation rules
  float cull_wf, cull_hf;
  float ds_rcp;  // RN(1 / ds_f): exact constant division (pcp_device.hpp div_by_ds)
  int32_t ds_fast;  // 1 when ds_f is in the range div_by_ds is proven for
  int32_t ds;
  int32_t img_w, img_h;
  int32_t cull_w, cull_h;
  int32_t mw, mh;  // cull_w/ds, cull_h/ds
  int32_t enable_zbuf;
  int32_t cull_mode;   // PCP_CULL_ZBUFFER / PCP_CULL_HPR_CANDIDATES (enable_zbuf is 0 with the latter; PCP_CULL_HPR runs
                       // the candidate filter here and the hull in pcp_hpr.hip)
  int32_t match_mode;  // PCP_MATCH_IDENTITY / PCP_MATCH_ROUNDTRIP / PCP_MATCH_RADIUS
  double cull_wd, cull_hd;  // cull size as fp64: bounds of hidden_points_removal's (int)u, (int)v rule
  float match_r2;      // f32(1e-5 * 1e-5): radiusSearch(epsilon) squared radius, PointCloudProcessor.cpp:482,571
  int32_t pretest;  // 1: run the conservative fp32 rejection test before the fp64 projection
  int32_t frames_bounded;  // 1: no entry of any keyframe's w2c exceeds 2^40 in magnitude (pcp_set_frames; see divide_xy_by_z)
  // fp32 copies for the rejection test (pcp_device.hpp surely_rejected): the coefficients (their absolute
  // values are source modifiers of the same registers) and the (u, v) box outside of which BOTH the cell rule
  // and the pixel rule reject, widened by 0.5 px
  float qfx, qfy, qcx, qcy;
  float qk1, qk2, qk3, qp1, qp2;
  float u_lo, u_hi, v_lo, v_hi;
};

// One keyframe: w2c / c2w 3x4 row-major fp32 (A1), the pose translation used by
// computeOrientationScore (hpp:207, B4) and an upper bound of the spectral norm of
// w2c's linear part (tile culling), and c2w.inverse() as the reference recomputes it in fp32 for every
// match (PointCloudProcessor.cpp:578).  192 B: three 64-B scalar-cache lines.
struct DevFrame {
  float w2c[12];
  float c2w[12];
  double px, py, pz;
  double norm_bound;
  float c2w_inv[12];
  float pad_[4];
};
static_assert(sizeof(DevFrame) == 192, "DevFrame layout");

// Per-point top-5 state, SoA over points: score[k][n], rgb[k][n], frame[k][n], count[n].
constexpr int kTopM = 5;  // PointCloudProcessor.cpp:615

struct TimingSlot {
  double total_ms = 0.0;
  int64_t launches = 0;
};

struct PendingEvent {
  hipEvent_t start, stop;
  int32_t kernel;
};

// seconds and bytes of the device allocations the CALLING THREAD has made (hipMalloc / hipFree inside DevBuf), for
// diagnostics.  One tally per thread: its reader, pcp_cloud_smooth_stream_begin, takes the difference over its own call on
// its own thread, so it sees that call's allocations and nothing of the contexts other host threads drive (the per-GPU
// threads of pcp_multi.hpp); a single-threaded caller gets what a process-wide tally gave.
struct AllocTally {
  double seconds = 0.0, bytes = 0.0;
};
inline AllocTally &alloc_tally() {
  static thread_local AllocTally t;
  return t;
}
struct AllocClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  ~AllocClock() { alloc_tally().seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

// Device memory, owned: freed by the destructor (on the device that is current then: pcp_destroy sets it before it deletes
// the context), by release() where memory is to go early, and by ensure() when it has to grow.  Moves, never copies.
template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t count = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), count(std::exchange(o.count, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      count = std::exchange(o.count, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= count && p) return hipSuccess;
    AllocClock clk;  // (device allocations cost 20-40 ms per GB on this platform: the diagnostics of the long calls report them)
    if (p) (void)hipFree(p);
    p = nullptr;
    count = 0;
    if (n == 0) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T));
    if (e == hipSuccess) {
      count = n;
      alloc_tally().bytes += static_cast<double>(n) * sizeof(T);
    }
    return e;
  }
  void release() {
    if (!p) return;
    AllocClock clk;
    (void)hipFree(p);
    p = nullptr;
    count = 0;
  }
};
static_assert(!std::is_copy_constructible_v<DevBuf<float>>, "DevBuf owns its memory");

// device PCD reader (pcp_ascii_parse.hip): what one piece of text in flight owns -- pinned staging, the text, the offsets of its
// '\n' bytes, the tile counts of the scan, four planes of parsed words, the result words (device and pinned) -- and the events
// that order its upload (staged), its kernels (parsed) and the download of its rows (drained) against the slot's next piece
struct AsciiParseSlot {
  void *stage = nullptr, *res_h = nullptr;
  size_t stage_bytes = 0;
  DevBuf<uint8_t> text;
  DevBuf<int32_t> end, tiles;
  DevBuf<uint32_t> out;
  DevBuf<unsigned long long> res;
  hipEvent_t staged = nullptr, parsed = nullptr, drained = nullptr;
  bool staged_live = false, parsed_live = false, drained_live = false;
};

// hidden_points_removal: the scratch of ONE keyframe's hull (pcp_hpr.hip).  The keyframes of a run are independent, so the
// whole-run pass keeps several of them in flight, each on a lane of its own: a stream, the buffers and a pinned readback
// into which the device publishes the candidates' count and bounds (the one host wait of a keyframe polls it).  Lane 0
// also serves the single-keyframe calls, on the context's stream.
struct HprLane {
  hipStream_t own_stream = nullptr;  // created on first use by the whole-run pass
  hipStream_t stream = nullptr;      // the stream the keyframe in flight was queued on
  unsigned long long seq = 0;        // sequence number of the keyframe whose counts the readback is waited for
  DevBuf<int32_t> index, i32, tiles;
  DevBuf<double> f64, cells_d, cont;  // cont: the searches k_hpr_tilt hands on (TiltCont records)
  DevBuf<uint8_t> state;
  DevBuf<unsigned long long> stats;
  void *readback = nullptr;  // pinned, kReadbackBytes
  // the keyframe between hpr_begin and hpr_finish
  bool busy = false;
  int32_t frame = -1;
  uint8_t *d_flags = nullptr;
  uint32_t *hull_plane = nullptr;
  uint32_t bit = 0;
  void release() {  // (the buffers free themselves)
    if (readback) (void)hipHostFree(readback);
    readback = nullptr;
    if (own_stream) (void)hipStreamDestroy(own_stream);
    own_stream = nullptr;
  }
};

// voxel-grid output (pcp_voxel_reduce.hip): the accumulator between pcp_voxel_reduce_begin and _end -- an open-addressing table
// (keys, three position sums and five 32-bit sums per slot), its device scalars, and the rows pcp_voxel_reduce_finish left
struct VoxelReduce {
  bool live = false, finished = false;
  bool labels_fixed = false, with_label = false;  // the first add fixes whether labels are accumulated
  float leaf = 0.0f;
  int64_t initial_slots = 0;  // 0: sized by the first add
  int64_t slots = 0, used = 0;  // used: keys in the table (a failed add may leave keys without rows behind)
  int64_t keyed = 0;            // keys that hold rows: `used` as the last successful add left it
  int64_t rows = 0, voxels = 0, growths = 0, partials = 0, atomics = 0;
  DevBuf<unsigned long long> keys, q, scalars;
  DevBuf<uint32_t> sums;
  DevBuf<float> out_xyz;
  DevBuf<uint8_t> out_rgb, out_label;
  DevBuf<uint32_t> out_count;
};

// orthographic maps (pcp_ortho.hip): the accumulator between pcp_ortho_begin and _end -- the frame, the key image and the
// payload image (12 B per pixel), its device scalars, and the source image pcp_ortho_finish left
struct OrthoMap {
  bool live = false, finished = false;
  bool labels_fixed = false, with_label = false;  // the first add fixes whether labels are held
  pcp_ortho_frame frame{};
  bool cyl = false;           // begun by pcp_ortho_begin_cyl: cyl_frame holds, and frame only its gsd, width and height
  pcp_cyl_frame cyl_frame{};
  int32_t fill_radius = 0;
  int64_t contributors = 0, atomics = 0, occupied = 0, filled = 0, adds = 0;
  DevBuf<unsigned long long> keys, scalars;
  DevBuf<uint32_t> payload;
  DevBuf<int32_t> source;  // per pixel: the pixel its values come from (-1: empty), after _finish
};

// surface defects of the live, finished map (pcp_ortho_defects.hip): the three layers, the table (16 words per kept region)
// and the counts of the last pcp_ortho_defects.  SD8: replaced by the next one; dropped by _finish, either begin, _end.
struct OrthoDefects {
  bool live = false;
  int64_t rows = 0;
  int64_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  DevBuf<int32_t> dev, region;
  DevBuf<uint8_t> cls;
  DevBuf<unsigned long long> table;
  void release() {
    live = false;
    rows = 0;
    dev.release(), region.release(), cls.release(), table.release();
  }
};

struct CrackMap;  // (the crack chain's header)

// planar facets (pcp_facets.hip): the labels (n, input order; -1: in no facet) and the table of the last pcp_facets -- ids,
// ten integers (points S1 S2) and the box as ordered integers per facet, ascending by id.  FA9: dropped by the next
// pcp_facets, pcp_estimate_normals and the uploads.
struct Facets {
  bool live = false;
  int64_t rows = 0;
  DevBuf<int32_t> label, ids;
  DevBuf<long long> table;
  DevBuf<uint32_t> box;
  void release() {
    live = false;
    rows = 0;
    label.release(), ids.release(), table.release(), box.release();
  }
};

// ---- the uniform grid of the radius searches (pcp_grid.hip; read by the MLS / SOR kernels, by the cell-wave search of
// local colour smoothing, normals, map comparison, map registration and the coarse registration's descriptors
// (pcp_cell_search.hpp), and by the per-lane walks of the neighbour table of PCP_MATCH_RADIUS and pcp_close_pairs) ---------
constexpr double kMaxGridCells = 536870912.0;      // 2^29: dense table of cell starts
constexpr double kMaxSparseCells = 34359738368.0;  // 2^35: bitmap (4 GiB) + running popcounts (2 GiB)
struct GridDesc {
  float minx, miny, minz, inv_cell;
  int32_t nx, ny, nz;
  int32_t reach;  // cells to visit on each side: ceil(r / cell)
  // Sparse form (nullptr: dense form, the table of cell starts has one entry per cell).  Grids of more than 2^29 cells keep
  // table entries for the OCCUPIED cells only; a bitmap with one bit per cell and the running popcount per 64-bit word
  // give the number of occupied cells before a cell -- its place in the table (1.5 bits per cell instead of 32).
  const unsigned long long *occ;
  const int32_t *occ_rank;
};

// ---- map registration (pcp_register.hip; DESIGN.md "Map registration", RG1): the transform of the comparison's base; made by the first registration call after
// pcp_compare_set_base, which resets it.  While it is live, base_xyz and the box hold the CURRENT rows (the original rows
// under T) and base0 the original ones.
struct RegisterState {
  bool live = false;
  rg::Transform T{{1.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  double c[3] = {0, 0, 0}, ell = 1.0;           // the pivot and the scale of the original box
  float mn0[3] = {0, 0, 0}, mx0[3] = {0, 0, 0};  // the original box
  DevBuf<float> base0;                           // the original planes
  DevBuf<unsigned long long> words;              // the partial slots, the folded sums, the box of a transform
  void release() {
    live = false;
    base0.release(), words.release();
  }
};

// ---- coarse registration (pcp_coarse.hip; DESIGN.md "Coarse registration", CG7): what the staged calls leave for the next.
// side[0]: the uploaded map (dropped with a compare result, at an upload, and by pcp_estimate_normals: its axes may have been the
// estimate that call replaces), side[1]: the base's ORIGINAL rows (dropped by
// pcp_compare_set_base).  A slot is row / stride; the host lists name the slots with a valid descriptor in ascending order.
struct CoarseSide {
  bool live = false;
  int64_t slots = 0, keypoints = 0;
  DevBuf<uint16_t> desc;   // 64 per slot
  DevBuf<uint32_t> total;  // n_i per slot
  DevBuf<uint8_t> state;   // 0: no keypoint, 1: keypoint without a valid descriptor, 2: valid
  DevBuf<float> xyz;       // 3 per slot
  std::vector<int32_t> valid_slot;
  std::vector<float> valid_xyz;
  void release() {
    live = false;
    slots = keypoints = 0;
    desc.release(), total.release(), state.release(), xyz.release();
    valid_slot.clear(), valid_xyz.clear();
  }
};
struct CoarseState {
  CoarseSide side[2];
  bool base_normals_live = false;  // CG1: the estimate of the base's normals (4 floats per row handed in)
  float base_normals_radius = 0.0f;
  DevBuf<float> base_normals;
  bool match_live = false;
  std::vector<int32_t> pairs;      // CG3: (base ordinal, map ordinal)
  std::vector<uint64_t> keys[2];   // best, second per valid keypoint: [0] of the map's, [1] of the base's
  void release_map() {
    side[0].release();
    match_live = false;
  }
  void release_base() {
    side[1].release();
    match_live = false;
    base_normals_live = false;
    base_normals.release();
  }
};

// ---- map comparison (pcp_compare.hip; DESIGN.md "Map comparison", MC8): the base survey and the last result ----------------
// The base (its finite rows as SoA planes and their tags: the caller's row with the epoch bit) lives from pcp_compare_set_base to
// pcp_compare_end or pcp_destroy; the result (input order of the map) from pcp_compare to the next upload.
struct CompareState {
  RegisterState reg;
  CoarseState coarse;
  bool base_live = false, result_live = false;
  int64_t n_base = 0, m_base = 0;  // rows handed in, finite rows kept
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};  // box of the finite rows
  DevBuf<float> base_xyz;      // planes of (m_base + 3) & ~3 floats
  DevBuf<uint32_t> base_tag;
  int64_t n = 0;               // points of the result
  DevBuf<float> distance, lod;
  DevBuf<uint8_t> status;
  DevBuf<long long> sums;      // 8 per point
  DevBuf<int32_t> direction;   // 3 per point
  int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  void release_result() {
    result_live = false;
    coarse.release_map();  // (CG7: the map's descriptors go with the cloud they were made from)
    n = 0;
    distance.release(), lod.release(), status.release(), sums.release(), direction.release();
  }
  void release() {
    release_result();
    base_live = false;
    n_base = m_base = 0;
    base_xyz.release(), base_tag.release();
    reg.release();
    coarse.release_base();
  }
};

// a cloud on the device the smoothing stages operate on (the uploaded map, or an
// intermediate of pcp_cloud_smooth); mn/mx = its bounding box
struct CloudView {
  const float *x, *y, *z;
  int64_t n;
  float mn[3], mx[3];
  // nullptr, or view index -> caller's point index: the uploaded map is walked through its
  // Morton-ordered copy (cell binning then permutes nearby memory only) and results are
  // reported under the caller's indices
  const int32_t *remap;
};

// ---- the two streams of the smoothing stage (pcp_mls.hip) ----------------------------------------------------------------
// the voxel grid of VOXEL_GRID_DILATION over a cloud's box (MLSVoxelGrid; voxel_of and the kernels are pcp_mls.hip's)
struct VoxelDesc {
  float bminx, bminy, bminz, vs;
  int32_t NX, NY, NZ, it;
  int64_t words;  // 32-bit words of the bitmap
};

// what an emission of dilated voxels needs beside the voxel set itself (ctx->v_*) and the fits (ctx->m_state)
struct VgdStream {
  VoxelDesc v;
  GridDesc g;            // the grid the emission searches (occ / occ_rank: ctx->g_occ, ctx->g_occ_rank)
  const int32_t *remap;  // the view's (ctx->perm, ctx->c_perm or nullptr)
  size_t plane;
  int32_t order_poly;
  int32_t bricks;         // 1: the voxel set is in bricks (chunks are runs of strips), 0: dense bitmap (runs of words)
  int32_t NBX, NBY, NBZ;
};
// a chunk of an emission: bitmap words (dense form; word0 a multiple of the scan tile) or strips (brick form) [word0, word1)
struct VgdChunk {
  int64_t word0, word1, voxels;
};

// pcp_cloud_smooth_stream_*: the whole chain with the trailing outlier removal over the chunked emission
struct SmoothStream {
  pcp_mls_params p;
  VgdStream S;
  CloudView cv1;  // the survivors of the first filter (planes in ctx->c_xyz)
  int64_t total_rows, kept_rows, rows_computed;
  double threshold, max_dx, min_margin;
  int32_t halo, redone;
  double sampled_dx;  // the largest displacement sweep 0 saw on its sample of the voxels (sizes the halo; max_dx proves it)
  double seconds[4];  // host clock of _begin: first filter + fit + voxel set, device allocations (inside the other three), sweep 0, sweep 1 + threshold
  double alloc_bytes;  // device memory allocated during _begin
};
// a chunk of the chain: whole planes [first_plane, last_plane] of the first voxel axis; its result rows are [row0, row0 + rows)
// of the upsampled cloud (and of ctx->css_dist)
struct ChainChunk {
  int64_t first_plane, last_plane, voxels, row0, rows;
};

// One stream: what it emits from, its chunks, the chunk its next _next emits.  Open: _next and _seek serve it.  Ended: a call
// replaced what it rests on (end_emission_stream / end_smoothing_streams below say which), or its own _end did; the chain's
// numbers stay readable for pcp_cloud_smooth_stream_stats.  Building: inside pcp_cloud_smooth_stream_begin (the chain only).
enum class StreamPhase { None, Building, Open, Ended };
template <typename Stream, typename Chunk>
struct StreamState {
  StreamPhase phase = StreamPhase::None;
  Stream of{};
  std::vector<Chunk> chunks;
  int64_t next = 0;
  bool open() const { return phase == StreamPhase::Open; }
  bool idle() const { return phase == StreamPhase::None || phase == StreamPhase::Ended; }  // neither open nor being built
  void end() {
    if (open()) phase = StreamPhase::Ended;
  }
};

}  // namespace pcp

struct pcp_context {
  int32_t device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // pinned host scratch for the small device-to-host readbacks (counts, bounds, tallies): a copy into pageable memory is
  // staged by the runtime and costs 20-30 us more per wait; 64 KB, allocated by pcp_create (nullptr: pageable fallback)
  void *readback = nullptr;
  static constexpr size_t kReadbackBytes = 65536;
  mutable std::string error;

  // configuration
  bool have_camera = false;
  bool uv_tame = false;  // p1, p2 are in the range the short distortion form is proven for (pcp_visit_forms.hpp): a condition
                         // of the common configuration, whose batched kernels run that form
  bool k3_dropped = false;  // k3 is a zero and the other constants are in the range for which the short form without the k3
                            // term is proven to give the same verdicts (pcp_visit_forms.hpp): the batched kernels of the common
                            // configuration run that form; any other camera keeps the term and stays in the common configuration
  pcp_camera camera{};
  pcp_cull_params cull{};
  pcp::DevCamera dcam{};

  // cloud: original order (per-keyframe drop-in calls) and spatially sorted copy
  // (batched run + MLS); perm[j] = original index of sorted point j.
  int64_t n = 0;
  int64_t nonfinite_points = 0;  // uploaded points with a NaN or infinite coordinate (the smoothing stages refuse them)
  pcp::DevBuf<float> xyz;    // x[n] y[n] z[n]
  pcp::DevBuf<float> sxyz;   // sorted x[n] y[n] z[n]
  pcp::DevBuf<int32_t> perm; // n
  pcp::DevBuf<int32_t> inv_perm;  // n: inv_perm[perm[j]] = j (un-permutes per-point results with coalesced stores)
  std::vector<float> host_min = {0, 0, 0}, host_max = {0, 0, 0};

  // frames
  int32_t n_frames = 0;
  std::vector<pcp_pose> poses;
  std::vector<pcp::DevFrame> hframes;
  pcp::DevBuf<pcp::DevFrame> frames;
  pcp::DevBuf<uint32_t> images;  // n_frames * img_h * img_w  (B | G<<8 | R<<16 | mask<<24)
  std::vector<uint8_t> image_set, mask_set;
  // pcp_upload_image_async: kUploadLanes streams of their own, taken in turn, each with one staging buffer (a stream
  // is in order): the copy of keyframe i + 1 crosses PCIe while keyframe i is packed, and both overlap the compute
  // stream.  An event per keyframe for the consumers, and an event of the compute stream that the next uploads wait
  // for when kernels that touch the texels were queued since the last one.
  static constexpr int kUploadLanes = 2;
  hipStream_t upload_stream[kUploadLanes] = {nullptr, nullptr};
  pcp::DevBuf<uint8_t> upload_stage[kUploadLanes];
  pcp::DevBuf<uint8_t> jpeg_planes[kUploadLanes];  // pcp_upload_image_jpeg: the lane's component planes (pcp_jpeg.hip)
  std::vector<hipEvent_t> image_event;   // per keyframe, recorded on its lane after its pack kernel
  std::vector<uint8_t> image_pending;    // 1: the consumer has not yet made its stream wait for image_event[f]
  std::vector<uint8_t> image_lane;       // lane of the keyframe's latest upload
  std::vector<uint64_t> image_seq;       // queue position of the keyframe's latest upload
  bool lane_must_wait[kUploadLanes] = {false, false};  // texels_idle not yet waited for on this lane
  uint64_t upload_seq = 0;   // queue position of the latest packed keyframe
  uint64_t upload_turn = 0;  // upload calls so far: the lanes take turns per call (a block of keyframes is one call)
  hipEvent_t texels_idle = nullptr;      // recorded on the compute stream
  bool texels_touched = false;           // compute-stream work on the texel buffer since the last wait
  // generateColorMap's 8-bit BGR -> HSV -> BGR round trip, fused into the pack kernel (pcp_set_image_adjust)
  bool adjust_images = false;
  float saturation_scale = 1.0f, brightness_scale = 1.0f;
  pcp::DevBuf<int32_t> hsv_tables;  // sdiv_table[256], hdiv_table180[256] (OpenCV RGB2HSV_b)
  // pcp_set_image_balance: CLAHE on V and a gamma table, in place on the packed texels behind the lane's pack kernel
  // (pcp_image_balance.hip).  The scratch is the lane's own: two lanes in flight never share it.
  pcp_balance_params balance{};     // stages == 0: off
  uint8_t balance_gamma[256] = {};  // IB8, built by pcp_set_image_balance
  uint64_t balance_seq = 0;         // settings so far: a lane copies the gamma table again when its own copy is older
  uint64_t balance_lane_seq[kUploadLanes] = {0, 0};
  pcp::DevBuf<uint32_t> balance_hist[kUploadLanes];  // [16 * 16][256] per-tile histograms, left zeroed by k_balance_lut
  pcp::DevBuf<uint8_t> balance_lut[kUploadLanes];    // [16 * 16][256] per-tile tables, then the gamma table's 256 bytes
  pcp::DevBuf<uint32_t> balance_image;               // pcp_image_balance: its scratch texels
  pcp::DevBuf<uint8_t> balance_bytes;                // pcp_image_balance: its BGR rows in and out

  // depth maps [n_frames][mh*mw] as uint view of positive floats
  pcp::DevBuf<uint32_t> depth;
  pcp::DevBuf<unsigned long long> depth_sq;  // per cell, min of the squared fp64 range (bit pattern) during a depth pass
  std::vector<uint8_t> depth_valid;
  bool depth_from_batch = false;  // pcp_set_depth_source: single-keyframe calls use the batched (merged) maps
  // pcp_depth_accum_*: the MIN of the maps of every cloud merged since the reset, [n_frames][mh*mw]; outlives the uploads
  // (a chunk of a streamed cloud is an index shard in time), dropped by pcp_set_camera / pcp_set_frames
  pcp::DevBuf<uint32_t> depth_accum;
  bool depth_accum_live = false;

  // tiles = wavefront-sized runs of 64 sorted points: bounds, two float4 each, (x, y, z, radius) of the bounding sphere and
  // (hx, hy, hz, 0), the half-extents of the world-axis box about the same centre, the groups of 16 tiles behind the tiles;
  // and the tile x keyframe visibility masks [tile][mask_words]
  int64_t n_tiles = 0;
  pcp::DevBuf<float> tile_bounds;
  pcp::DevBuf<uint32_t> tile_mask, group_mask;
  pcp::DevBuf<uint32_t> tile_inside;  // pairs whose whole tile images inside the acceptance box (a hint: skip the pre-test)
  int32_t mask_words = 0;
  // longest-work-first order of the tiles for the batched passes (pcp_colour.hip k_work_*)
  pcp::DevBuf<int32_t> tile_work, tile_order, work_hist;
  bool tile_order_live = false;

  // per-point colour state (sorted order) and packed results
  pcp::DevBuf<float> top_score;     // 5*n
  pcp::DevBuf<uint32_t> top_rgb;    // 5*n
  pcp::DevBuf<int32_t> top_frame;   // 5*n
  pcp::DevBuf<int32_t> view_count;  // n
  // packed results in input order, double-buffered so that the device-to-host copy of one
  // run (copy stream) overlaps the kernels of the next
  pcp::DevBuf<uint32_t> rgba2[2];
  int32_t rgba_cur = 0;
  hipStream_t copy_stream = nullptr;
  hipEvent_t result_ready[2] = {nullptr, nullptr}, copy_done[2] = {nullptr, nullptr};
  bool copy_pending[2] = {false, false};
  bool colour_state_live = false;
  bool colour_result_live = false;
  // fused segmentation labels (pcp_set_label_fusion): label | hits<<8 | views<<16 per point, input order, written next to
  // the colour word by the label form of the colour kernels; one buffer (not double-buffered); word n is the range flag
  bool label_fusion = false;
  bool labels_live = false;
  pcp::DevBuf<uint32_t> labels;
  // exposure gains (pcp_exposure.hip): one fp32 gain per keyframe for the gained finalise (pcp_set_frame_gains; dropped by
  // pcp_set_frames), the pair matrices n | sum | counters of the last pcp_view_pair_stats and its counters on the host
  bool gains_set = false;
  pcp::DevBuf<float> gains_dev;
  pcp::DevBuf<unsigned long long> pair_stats;
  int64_t pair_counters[5] = {0, 0, 0, 0, 0};
  bool pair_counters_live = false;

  // voxel-grid output: belongs to the context, not to the cloud or the camera (only pcp_voxel_reduce_begin / _end and pcp_destroy drop it)
  pcp::VoxelReduce voxel_reduce;
  // orthographic maps: the same lifetime (only pcp_ortho_begin / _end and pcp_destroy drop it)
  pcp::OrthoMap ortho;
  pcp::OrthoDefects ortho_defects;

  // geometry maps (pcp_normals.hip): normal + curvature (float4) and neighbour count per point of the uploaded cloud, input
  // order, dropped by the uploads; the key image and the four output images of pcp_frame_geometry (allocated on first use)
  bool gn_live = false;
  float gn_radius = 0.0f;
  pcp::DevBuf<float> gn_normal;
  pcp::DevBuf<int32_t> gn_count;
  pcp::DevBuf<unsigned long long> gm_keys;
  pcp::DevBuf<uint32_t> gm_out;  // index | range | xyz_cam (3) | normal_cam (3), W*H words each
  // planar facets of the map: made from the cloud and the normals above, and dropped with either
  pcp::Facets facets;

  // map comparison: the base survey (kept across uploads) and the last result (dropped by the uploads)
  pcp::CompareState compare;

  // mask distance maps (pcp_mask_edt.hip), for one chunk of keyframes, allocated on first use: the background bits of the
  // column segments, the column words, and the two result images
  pcp::DevBuf<unsigned long long> md_bits;
  pcp::DevBuf<uint32_t> md_col, md_d2;
  pcp::DevBuf<int32_t> md_nearest;

  // crack width maps (the per-keyframe width unit), allocated on first use: the ten summed-area planes of the origin moments
  // (modulo 2^64) with the column stage's segment sums behind them, and the outputs a call asked for
  pcp::DevBuf<unsigned long long> cw_sat;
  pcp::DevBuf<uint8_t> cw_flags;
  pcp::DevBuf<int32_t> cw_i32;     // edges (4 per pixel) | w2d2
  pcp::DevBuf<float> cw_f32;       // plane (4 per pixel) | width | points (6 per pixel)
  pcp::DevBuf<long long> cw_moments;  // 13 per pixel

  // the crack chain on the map -- the fused widths and the tables of the cracks' components, lengths and skeletons -- with its
  // lifetime rules: pcp::CrackMap, defined in the chain's own header and allocated by pcp_create
  std::unique_ptr<pcp::CrackMap> crack;

  // PCP_MATCH_RADIUS (pcp_match.hip): the neighbour table within R_c, built by the first colour pass in that mode and
  // dropped by pcp_upload_cloud / pcp_set_frames (E depends on both).  Set A = points whose row holds another point.
  bool match_live = false;
  double match_e = 0.0, match_rc = 0.0;  // E (proven round-trip displacement bound) and R_c, metres
  float match_e2 = 0.0f;                 // E^2 rounded up: the colour pass counts samples displaced further
  int64_t match_a = 0;                   // |A|
  int64_t match_entries = 0;             // sum over A of the row lengths
  pcp::DevBuf<uint8_t> match_in_a;       // n flags, Morton order
  pcp::DevBuf<int32_t> match_list;       // the points of A (Morton indices, ascending)
  pcp::DevBuf<int64_t> match_off;        // |A| + 1 row offsets
  pcp::DevBuf<int32_t> match_cols;       // rows: Morton indices, each row sorted by input index, the point itself included
  pcp::DevBuf<unsigned long long> match_moved;  // samples displaced further than E by the last colour pass

  // scratch for the single-frame calls
  pcp::DevBuf<int32_t> s_cell, s_pixel;
  pcp::DevBuf<float> s_range, s_cam;
  pcp::DevBuf<uint8_t> s_keep;
  pcp::DevBuf<uint32_t> s_u32;
  pcp::DevBuf<unsigned long long> s_counter;
  pcp::DevBuf<int32_t> s_tiles;

  // hidden_points_removal (pcp_hpr.hip): candidate list, flipped points (candidate and cell order), cells, states
  static constexpr int kHprMaxLanes = 8;
  pcp::HprLane hpr_lane[kHprMaxLanes];
  int32_t hpr_last_lane = 0;  // whose tallies pcp_hpr_stats reads
  hipEvent_t hpr_fork = nullptr, hpr_join[kHprMaxLanes] = {};
  pcp::DevBuf<uint32_t> hull_bits;  // whole run: uint32[(F + 31) / 32][n], bit f & 31 of word (f >> 5, j) = point j (Morton
                                    // order) is a hull vertex of keyframe f
  std::vector<uint8_t> hull_valid;  // per keyframe: hull bits imported (index shards)
  int64_t hpr_stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool hpr_stats_pending = false;  // the tallies of the last hull still sit on the device (h_stats)

  // MLS: uniform grid (cell id / in-cell rank per point, cell starts, cell-sorted
  // order + coordinates), per-input-point results, compacted outputs
  pcp::DevBuf<int32_t> g_cell, g_rank, g_start, g_order;
  pcp::DevBuf<unsigned long long> g_occ;  // sparse grids: one bit per cell
  pcp::DevBuf<int32_t> g_occ_rank;        // ... and the set bits before each 64-bit word
  pcp::DevBuf<float> g_xyz;      // cell-sorted x[n] y[n] z[n]
  pcp::DevBuf<float> m_tmp;      // 8 floats per input point (xyz, normal, curvature, pad: one 32-byte sector), input order
  pcp::DevBuf<float> s_dist;     // StatisticalOutlierRemoval: mean kNN distance per point
  pcp::DevBuf<double> m_state;   // per-point MLSResult (mean, axes, c_vec ...) for upsampling
  double slp_radius = 0.05, slp_step = 0.01;  // SAMPLE_LOCAL_PLANE (pcp_set_mls_local_plane; PointCloudProcessor.cpp:74-75)
  pcp::DevBuf<float> slp_table;  // its sample table, u v interleaved, for slp_table_of (radius, step)
  double slp_table_of[2] = {0.0, 0.0};
  pcp::DevBuf<int32_t> c_perm;   // pcp_cloud_smooth SAMPLE_LOCAL_PLANE: spatial order of the first filter's survivors
  pcp::DevBuf<uint8_t> m_flag;   // n
  pcp::DevBuf<double> m_sums;    // SOR statistics
  pcp::DevBuf<int32_t> c_index;  // pcp_cloud_smooth: survivors of the 1st SOR (indices into the uploaded cloud)
  int32_t sor_partial_slab = -1, sor_partial_slabs = -1;  // the slab of the cell order whose mean distances the last pcp_sor_partial left in s_dist
  bool sor_distances_live = false;  // s_dist holds the mean distances of the last pcp_sor (caller's order)
  pcp::DevBuf<uint8_t> c_mark;    // pcp_cloud_smooth: per uploaded point, survives the whole chain
  pcp::DevBuf<int32_t> c_where;   // ... and the result row that holds it
  pcp::DevBuf<float> c_xyz, c_xyz2;  // pcp_cloud_smooth: intermediate clouds (SoA)
  pcp::DevBuf<uint32_t> v_bitmap;  // dilated voxel set: the bits of the occupied bricks (or the dense bitmap over the bounding box, PCP_VGD_DENSE=1)
  pcp::DevBuf<int32_t> v_offsets;  // set bits per strip of the brick form (per tile of 1024 words of the dense bitmap)
  pcp::DevBuf<uint32_t> v_occ;     // brick form: one bit per brick place
  pcp::DevBuf<int32_t> v_rank;     // brick form: occupied places before each word of v_occ
  pcp::DevBuf<unsigned long long> v_plane;  // brick form: voxels per plane ix
  pcp::DevBuf<int64_t> v_vox;      // occupied voxels (linear index) in key order
  pcp::DevBuf<float> mls_xyz, mls_normal, mls_curv;
  pcp::DevBuf<int32_t> mls_index;
  // second set: pcp_cloud_smooth compacts the survivors of its last SOR into it and swaps the sets
  pcp::DevBuf<float> mls_alt_xyz, mls_alt_normal, mls_alt_curv;
  pcp::DevBuf<int32_t> mls_alt_index;
  int64_t mls_count = 0;
  bool mls_result_live = false;  // a smoothing call has left mls_count rows (0 included) since the latest upload
  hipEvent_t handoff = nullptr;  // pcp_upload_cloud_from_result: recorded on this (source) context's stream
  pcp::DevBuf<uint8_t> cc_out;   // pcp_colour_compact: the gathered rows (xyz | rgb | label) before they leave the device
  // device PCD writer (pcp_ascii.hip): host rows uploaded by pcp_ascii_rows, a length per row, the 64-bit prefix of the tiles'
  // bytes (+ the window edges), one window of text
  pcp::DevBuf<uint8_t> ascii_in, ascii_len, ascii_text;
  pcp::DevBuf<unsigned long long> ascii_tiles;
  // device PCD reader (pcp_ascii_parse.hip): two slots a window's pieces alternate between, an upload and a download stream
  pcp::AsciiParseSlot parse_slot[2];
  hipStream_t parse_up = nullptr, parse_down = nullptr;
  // pcp_mls_stream_*: the plan of a chunked VOXEL_GRID_DILATION emission
  pcp::StreamState<pcp::VgdStream, pcp::VgdChunk> emission;
  // pcp_cloud_smooth_stream_*: the whole chain with the trailing outlier removal over the chunked emission
  pcp::StreamState<pcp::SmoothStream, pcp::ChainChunk> chain;
  pcp::DevBuf<float> css_dist;      // mean kNN distance of EVERY row of the dilated cloud (4 B x ~3.8e9 at C3)
  pcp::DevBuf<float> s_kth;         // per row of a chunk: bound of the squared distance to its (k + 1)-th nearest
  pcp::DevBuf<uint32_t> css_words;  // device scalars of the stream (max displacement, margins, counts)
  double css_ball = 0.0;            // the chain's alone: the trailing filter's ball, in (k + 1) rows by the voxel structure's density bound, as the last chunks left it (0: default); outlives a stream, reset by an upload
  double sor_redo_fraction = 0.0;  // diagnostic: share of points the SOR selection kernel handed to the heap kernel

  // NID stage (section 8 f1): per-point intensity, per-keyframe culled clouds in camera
  // coordinates (x, y, z, intensity), chunked so that a workgroup sees one keyframe
  pcp::DevBuf<float> intensity;
  bool have_intensity = false;
  pcp::DevBuf<float> nid_pts;        // float4 per entry, NaN intensity = padding
  pcp::DevBuf<int32_t> nid_chunk_kf; // keyframe of every chunk
  pcp::DevBuf<double> nid_hist;      // [keyframe][bins*bins*7 + bins]
  int64_t nid_chunks = 0, nid_points = 0;
  int32_t nid_frames = 0;
  int32_t nid_hist_bins = 0;  // bins of the histograms pcp_nid_accumulate left in nid_hist

  // measurement
  bool timing = false;
  pcp::TimingSlot slots[PCP_K_COUNT];
  std::vector<pcp::PendingEvent> pending;
  std::vector<hipEvent_t> event_pool;
};

namespace pcp {

// ---- the grid's device side (GridDesc is above the context) ----
// number of occupied cells before cell c (sparse form)
__device__ __forceinline__ int32_t cell_rank(const GridDesc &g, int64_t c) {
  const unsigned long long bits = g.occ[c >> 6];
  return g.occ_rank[c >> 6] + static_cast<int32_t>(__popcll(bits & ((1ull << (c & 63)) - 1ull)));
}

// Entry (zz, yy, xx) of the table of cell starts = number of points in the cells before that cell (xx may be nx: the
// first cell of the next row).  The cells of a row are consecutive in either form, so start(x0) .. start(x1 + 1) is the
// run of candidates of the cells x0 .. x1 of a row.
__device__ __forceinline__ int32_t cell_start(const GridDesc &g, const int32_t *__restrict__ start, int32_t zz, int32_t yy,
                                              int32_t xx) {
  if (!g.occ) return start[(zz * g.ny + yy) * g.nx + xx];
  return start[cell_rank(g, (static_cast<int64_t>(zz) * g.ny + yy) * g.nx + xx)];
}

__device__ __forceinline__ void grid_coords(const GridDesc &g, float x, float y, float z, int32_t &ix, int32_t &iy,
                                            int32_t &iz) {
  ix = min(max(static_cast<int32_t>(floorf((x - g.minx) * g.inv_cell)), 0), g.nx - 1);
  iy = min(max(static_cast<int32_t>(floorf((y - g.miny) * g.inv_cell)), 0), g.ny - 1);
  iz = min(max(static_cast<int32_t>(floorf((z - g.minz) * g.inv_cell)), 0), g.nz - 1);
}

// uniform grid over a cloud view, cell edge >= `cell`, reach = ceil(radius / cell): the table of cell starts in
// ctx->g_start, the view's points in cell order in ctx->g_order (view indices; ascending inside a cell) and ctx->g_xyz
// (SoA planes of (n + 3) & ~3 floats).  Coordinates must be finite.
// geometry_only: just the grid description and a large enough cell table (the density probe of sor_run fills it).
int build_grid(pcp_context *ctx, const CloudView &cv, float cell, float radius, GridDesc *out, bool geometry_only = false);
// Which call ends which stream.  The emission stream searches the context's grid: a call that rebuilds the grid ends it (the
// outlier removal: sor_run).  The chain rebuilds its grid per chunk but rests on the cloud, the first filter's survivors and
// the fits: a call that replaces those ends both (an upload: store_cloud; a fit: mls_run), and so does every radius stage
// (build_radius_grid).  build_grid itself ends neither: the chain's own chunks go through it.  pcp_cloud_smooth_stream_end ends
// the chain alone; the two _begin calls end the other kind through the fit they run.
inline void end_emission_stream(pcp_context *ctx) { ctx->emission.end(); }
inline void end_smoothing_streams(pcp_context *ctx) {
  ctx->emission.end();
  ctx->chain.end();
}
// The NID stage's prepared state (the gathered camera-frame points, their chunks, the histograms) belongs to the cloud, the
// intensities, the keyframes and the camera it was gathered with: a call that replaces one of them drops it (store_cloud,
// pcp_upload_intensity, pcp_set_frames, pcp_set_camera), and the evaluation calls refuse until pcp_nid_prepare ran again.
// Not the images (read live at every evaluation) and not the depth source or accumulator (set before the prepare).
inline void nid_release(pcp_context *ctx) {
  ctx->nid_frames = 0;
  ctx->nid_chunks = 0;
  ctx->nid_points = 0;
  ctx->nid_hist_bins = 0;
}

// ---- the front end of the stages that search a fixed radius around every point of the uploaded cloud (pcp_grid.hip) ----
// the uploaded cloud as a view: its Morton-ordered copy and the host box of its finite coordinates; with_remap: results
// go under the caller's indices (remap = perm), else under Morton indices (remap = nullptr)
CloudView uploaded_view(const pcp_context *ctx, bool with_remap);
// per-call scratch of finite_view: released when the call that owns it returns
struct FiniteScratch {
  DevBuf<uint8_t> flag;
  DevBuf<int32_t> pos, vremap;
  DevBuf<float> vxyz;
};
// The finite points of the uploaded cloud as a view (the grid needs finite coordinates).  A cloud without non-finite points:
// uploaded_view as it is, *pos = nullptr (view and Morton indices are the same).  Otherwise the finite points are flagged, compacted and gathered into `s`:
// *pos (pos nullable) = view index -> Morton index, remap = view index -> caller's index (with_remap) or nullptr; cv->n
// may be 0.  timing_slot: the PCP_K_* slot its launches are charged to, or -1 for none.
int finite_view(pcp_context *ctx, bool with_remap, int32_t timing_slot, FiniteScratch &s, CloudView *cv,
                const int32_t **pos = nullptr);
// The grid of a radius stage over cv (cv.n > 0): ends the streams and the pcp_sor_partial that rest on the old grid, then
// build_grid with cell edge max(radius * 1.001, the edge that gives ~8 cells per point), reach 1.
int build_radius_grid(pcp_context *ctx, const CloudView &cv, float radius, GridDesc *out);
// a radius stage may have taken the sparse grid: its bitmap is not kept when it is larger than 2^25 words
void drop_large_grid_bitmap(pcp_context *ctx);

int set_error(const pcp_context *ctx, int code, const char *fmt, ...);
// one per translation unit with kernels: forces the runtime to load that unit's code object (pcp_context.hip preload_code_objects)
hipError_t preload_colour();
hipError_t preload_mls();
hipError_t preload_grid();
hipError_t preload_nid();
hipError_t preload_hpr();
hipError_t preload_colour_smooth();
void set_global_error(const char *fmt, ...);

#define PCP_HIP_TRY(ctx, expr)                                                                       \
  do {                                                                                               \
    hipError_t e__ = (expr);                                                                         \
    if (e__ != hipSuccess)                                                                           \
      return pcp::set_error((ctx), e__ == hipErrorOutOfMemory ? PCP_ERR_NOMEM : PCP_ERR_DEVICE,       \
                            "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

// RAII bracket: records start/stop events around a launch when timing is on.
struct LaunchTimer {
  pcp_context *ctx;
  PendingEvent ev{};
  bool active = false;
  LaunchTimer(pcp_context *c, int32_t kernel);
  ~LaunchTimer();
};

int drain_timing(pcp_context *ctx);

// make ctx->stream wait for the asynchronous uploads of keyframes [f0, f1) that are still in flight, and note that
// the compute stream is about to touch the texel buffer (pcp_colour.hip)
int wait_images(pcp_context *ctx, int32_t f0, int32_t f1);

// One image upload call (pcp_colour.hip upload_texels): the lane, event and keyframe bookkeeping is upload_texels'; what
// turns the caller's source into texels is the TexelSource's.  validate runs first (no device work queued before it
// succeeds), stage once per call on the lane's stream, pack once per keyframe frame + k of the call.
struct TexelSource {
  virtual int validate(pcp_context *ctx, const char *who) = 0;
  virtual int stage(pcp_context *ctx, int lane, hipStream_t us) = 0;
  virtual int pack(pcp_context *ctx, int lane, hipStream_t us, int32_t k, uint32_t *dst, int32_t clear_mask,
                   const int32_t *hsv_tables) = 0;
};
// the pack kernel for decoded BGR8 rows (pcp_colour.hip: k_pack_bgr16 where rows and width allow, else k_pack_bgr), and the
// OpenCV tables of the HSV conversion on the device
void pack_bgr_texels(hipStream_t s, const uint8_t *src, int64_t row_stride_bytes, int32_t w, int32_t h, uint32_t *dst, int32_t clear_mask,
                     const int32_t *hsv_tables, float sat_scale, float val_scale);
int ensure_hsv_tables(pcp_context *ctx);

// The image balance of one keyframe's texels, in place, on a lane's stream with that lane's scratch (pcp_image_balance.hip).
struct BalanceRun {
  pcp_balance_params params;
  const uint8_t *gamma_host;   // 256 bytes, copied to the lane when gamma_stale
  bool gamma_stale;
  const int32_t *hsv_tables;   // device; needed with PCP_BALANCE_CLAHE or adjust
  bool adjust;                 // IB9: pcp_set_image_adjust's round trip last
  float sat_scale, val_scale;
  bool timed;                  // PCP_K_MISC (the context's stream only)
  uint32_t *out_hist;          // host, nullable: the raw histograms
  uint8_t *out_lut;            // host, nullable
};
int balance_check(pcp_context *ctx, const char *who, const pcp_balance_params &p, int32_t w, int32_t h);  // IB3's refusal
int balance_scratch(pcp_context *ctx, int lane, hipStream_t s);
int balance_texels(pcp_context *ctx, int lane, hipStream_t s, const BalanceRun &run, int32_t w, int32_t h, uint32_t *texels);
hipError_t preload_image_balance();

// count > 1 only for a block of keyframes staged together (pcp_upload_images_block); wait: synchronise the lane
int upload_texels(pcp_context *ctx, const char *who, int32_t frame, int32_t count, bool block, bool wait, TexelSource &src);

// the upload's spatial order of n > 0 device points (pcp_context.hip): box, Morton keys, stable radix sort, ordered copy
int spatial_order(pcp_context *ctx, const float *dx, const float *dy, const float *dz, int64_t n, int32_t *perm, float *sx,
                  float *sy, float *sz, int32_t *inv_perm, float mn[3], float mx[3], unsigned long long *out_nonfinite);

// ordered compaction of a device byte-flag array (pcp_colour.hip): index list (nullable) + count
int compact_flags(pcp_context *ctx, const uint8_t *flags, int64_t n, int32_t *out_index, int64_t capacity,
                  int64_t *count);

// ViewCulling::cull of one keyframe on the device: ordered index list of kept points (pcp_colour.hip)
int cull_frame_indices(pcp_context *ctx, int32_t frame, int32_t *d_index, int64_t capacity, int64_t *count);

// hidden_points_removal's hull over the candidate flags of one keyframe (pcp_hpr.hip): flags (input order, device)
// in: 1 = candidate; out: 1 = hull vertex
int hpr_run(pcp_context *ctx, int32_t frame, uint8_t *d_flags, uint32_t *hull_plane, uint32_t bit);
// the hulls of keyframes [f0, f1) into the (cleared) whole-run bits, `lanes` keyframes in flight on streams of their own
int hpr_run_range(pcp_context *ctx, int32_t f0, int32_t f1, int32_t lanes, const uint32_t *tile_mask = nullptr);

// smoothColorsWithLocalRegion (pcp_colour_smooth.hip): the packed words d_in (device, input order, n = ctx->n) smoothed into
// d_out (device; d_in == d_out allowed); *out_has_count = words of d_out with the has bit.  Synchronises the stream.
bool smooth_radius_ok(float radius);  // LS7: finite, 0 < radius <= 1
int colour_smooth_words(pcp_context *ctx, float radius, const uint32_t *d_in, uint32_t *d_out, int64_t *out_has_count);

// PCP_MATCH_RADIUS (pcp_match.hip): builds the neighbour table if it is not live (E, R_c, flags, list, rows)
int match_table_prepare(pcp_context *ctx);
void match_table_release(pcp_context *ctx);
hipError_t preload_match();
hipError_t preload_jpeg();
hipError_t preload_stream_colour();
hipError_t preload_ascii();
hipError_t preload_ascii_parse();
hipError_t preload_exposure();
hipError_t preload_voxel_reduce();
hipError_t preload_normals();
hipError_t preload_mask_edt();
hipError_t preload_ortho();
hipError_t preload_ortho_texture();
hipError_t preload_facets();
hipError_t preload_ortho_defects();
hipError_t preload_compare();
hipError_t preload_register();
hipError_t preload_coarse();
// the normals stage's own search and solve over any view (pcp_normals.hip): out_normal (float4) and out_count under the view's
// remap, the caller's to clear; the map's live estimate is not touched.  *out_most: the largest neighbour count.
int normals_of_view(pcp_context *ctx, const CloudView &cv, float radius, const char *who, float *out_normal4, int32_t *out_count,
                    int64_t *out_most);
// the device parts of pcp_mask_edt (one keyframe, with nearest) and pcp_frame_geometry under the caller's name: checks and
// kernels, the results left in md_bits / md_d2 / md_nearest and gm_out / s_counter[0]; no copy, no synchronisation
int mask_edt_device(pcp_context *ctx, const char *who, int32_t frame, int32_t threshold);
// k_md_columns and k_md_rows on a caller's bit image of one w x h picture (bit j of word [s][x] = pixel (x, 64 s + j) is
// background; segs = ceil(h / 64)): column words into `col`, then d2 and nearest (nullable), w * h words each, all device
// memory of the caller's (pcp_ortho.hip fills a map through them).  Queues on ctx->stream; no checks, no synchronisation.
int mask_edt_of_bits(pcp_context *ctx, const unsigned long long *bits, int32_t w, int32_t h, int32_t segs, uint32_t *col,
                     uint32_t *out_d2, int32_t *out_nearest);
// (*out_contributors, nullable: the length of the keyframe's list, which frame_contributors left in ctx->s_cell)
int frame_geometry_device(pcp_context *ctx, const char *who, int32_t frame, bool with_normals, int64_t *out_contributors = nullptr);
// reductions over the 64 lanes of a wavefront (every lane gets the result)
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o, 64)));
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o, 64)));
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(v), o, 64));
  return v;
}
void normals_release(pcp_context *ctx);   // the normals of the cloud that is being replaced (the uploads)
// the list pcp_frame_visible reports for one keyframe (pcp_colour.hip): ascending input indices in ctx->s_cell, *m of them;
// checks the context and the keyframe as that call does, under the caller's name
int frame_contributors(pcp_context *ctx, const char *who, int32_t frame, int64_t *m);
// EG5 (pcp_exposure.hip): the packed result from the live top-5 state under ctx->gains_dev (and the label words with label
// fusion on); ctx->n > 0, a live state and set gains are the caller's to check
int finalise_gained(pcp_context *ctx, uint32_t *result);
void ascii_parse_release(pcp_context *ctx);  // the reader's pinned memory, streams and events (pcp_destroy)

// removePointsWithNoColor's index list (pcp_stream_colour.hip): the rows of the current colour result whose has bit is set,
// input order, into ctx->s_cell; *m = their number.  ctx->n > 0 and a live colour result are the caller's to check.
int colour_compact_indices(pcp_context *ctx, int64_t *m);

inline int64_t div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace pcp
