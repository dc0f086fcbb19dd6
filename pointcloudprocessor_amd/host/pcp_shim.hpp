// pcp_shim.hpp -- C++ host shim above the C ABI (include/pcp_hip.h).
//
// Mirrors the reference's operator interface for the hot path so that the
// existing C++ binary keeps its call structure:
//
//   pcp_amd::ViewCulling::cull        <- vlcal::ViewCulling::cull           (view_culling.hpp:34)
//   pcp_amd::Colorizer::colorize      <- pcdColorizationAndSmooth inner loop (PointCloudProcessor.cpp:488-596)
//   pcp_amd::Colorizer::frameVisible  <- generateColorMap + generateSegmentMap (:531-551)
//   pcp_amd::CloudSmooth::process     <- CloudSmooth::process               (cloudSmooth.cpp:77-185)
//
// Error convention: the ABI never throws; this shim rethrows std::runtime_error
// so that main.cpp:64-68 still maps failures to exit code -2.
// Header-only, depends on the C ABI alone (no PCL / Eigen / OpenCV types): the
// caller passes raw pointers taken from its own containers.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "pcp_hip.h"

namespace pcp_amd {

// The voxel-grid output (pcp_hip.h, "voxel-grid output"): one row per occupied voxel, in key order
struct VoxelCloud {
  std::vector<float> xyz;       // 3 per row: the centroid
  std::vector<uint8_t> rgb;     // 3 per row: the mean colour
  std::vector<uint8_t> label;   // mean fused label per row (asked for and accumulated), else empty
  std::vector<uint32_t> count;  // rows of the coloured cloud in the voxel
};

// An orthographic map (pcp_hip.h, "orthographic maps"): layers of frame.width x frame.height, row-major
// surface defects of a finished orthographic map (DESIGN.md "Surface defects on ortho maps"): the eight counts, the layers
// and 16 integers per kept region (pcp_hip.h)
struct OrthoDefects {
  int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // kept, dropped, hollow px, bulge px, unsupported, refused, first pass, surface
  std::vector<int32_t> dev;     // quanta of 2^-20 m
  std::vector<uint8_t> cls;     // 0, 1 hollow, 2 bulge
  std::vector<int32_t> region;  // 0: none, else 1..kept
  std::vector<int64_t> rows;    // 16 per kept region
};

struct OrthoMap {
  pcp_ortho_frame frame{};
  int64_t contributors = 0, occupied = 0, filled = 0;
  std::vector<uint32_t> index;   // global index of the point behind the pixel, 0xFFFFFFFF: empty
  std::vector<float> depth;      // its depth along n, 0 when empty
  std::vector<uint8_t> rgb;      // 3 per pixel
  std::vector<uint8_t> label;    // fused label per pixel (asked for and held), else empty
  std::vector<uint8_t> status;   // 0 empty, 1 direct, 2 filled
  std::vector<int32_t> source;   // linear index of the pixel the values come from, -1: empty
};

// An orthophoto (pcp_hip.h, "orthophotos"): layers of `width` x `height` fine pixels, row-major, of the rectangle the call asked for
struct OrthoPhoto {
  int32_t width = 0, height = 0;
  int64_t surface = 0, textured = 0, unseen = 0, skipped_pairs = 0;
  std::vector<uint8_t> rgb;     // 3 per fine pixel, from the keyframe images
  std::vector<uint8_t> mask;    // the mask byte of the best view's texel
  std::vector<uint8_t> status;  // 0 no surface, 1 textured, 2 surface that no view lists
  std::vector<int16_t> view;    // keyframe of the best view, -1: not textured
  std::vector<uint8_t> count;   // listed views, at most 255
};

// The geometry maps of one keyframe (pcp_hip.h, "geometry maps"): images of `width` x `height`, row-major
struct GeometryMaps {
  int32_t width = 0, height = 0;
  int64_t pixels = 0;              // occupied
  std::vector<int32_t> index;      // input index of the point behind the pixel, -1: empty
  std::vector<float> range;        // distance_mask
  std::vector<float> xyz_cam;      // 3 per pixel: points_3d_mask
  std::vector<float> normal_cam;   // 3 per pixel: norm_mask (asked for), else empty
};

// The mask distance maps of `count` keyframes (pcp_hip.h, "mask distance maps"): images of `width` x `height`, row-major,
// one keyframe after the other
struct MaskDistance {
  int32_t width = 0, height = 0, count = 0;
  std::vector<uint32_t> d2;       // exact squared distance to the nearest background pixel (0xFFFFFFFF: the mask has none)
  std::vector<int32_t> nearest;   // its linear index, the lowest of equally near ones (-1: none); empty when not asked for
};

// The crack width maps of one keyframe (pcp_hip.h, "crack width maps"): images of `width` x `height`, row-major
struct CrackWidth {
  int32_t width = 0, height = 0;
  int64_t sites = 0, widths = 0;   // pixels with the SITE / the WIDTH flag
  std::vector<uint8_t> flags;      // bit 0 SITE, 1 CENTRE, 2 NEAR, 3 FAR, 4 PLANE, 5 RAYS, 6 WIDTH
  std::vector<int32_t> edges;      // 4 per pixel: the near and the far edge point, doubled; -1: missing
  std::vector<float> width_m;      // metres, 0 without WIDTH
  std::vector<float> points;       // 6 per pixel: the two edge points in camera coordinates
  std::vector<float> plane;        // 4 per pixel: unit normal facing the camera and -n.c (asked for), else empty
};

// The crack widths of a set of keyframes on the map, and the map's cracks (pcp_hip.h, "crack widths on the map"): per map
// point in input order, and one row per crack, ascending by id
// planar facets of the map (Device::facets; DESIGN.md, "Planar facets"): one row per face of the structure
// what pcp_compare leaves per point of the uploaded map (DESIGN.md "Map comparison")
struct MapComparison {
  std::vector<float> distance, lod;  // metres; 0 where status < 3
  std::vector<uint8_t> status;       // MC6
  int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// what pcp_compare_register leaves (DESIGN.md "Map registration", RG8)
struct Registration {
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // row-major: base -> map
  std::vector<double> log;  // 5 per iteration: pairs, rms, dof, |omega| ell, |dt|
  int32_t status = 0, iterations = 0, dof = 0;
  int64_t pairs = 0;
  double rms = 0.0;  // of the last iteration, metres: what a caller may pass as reg_error
};

struct Facets {
  int64_t facet_points = 0, components = 0;
  std::vector<int32_t> label;   // per map point: the facet's id (the lowest input index of its points), -1: in no facet
  std::vector<int32_t> ids;     // ascending
  std::vector<int64_t> rows;    // 10 per facet: points, S1 x y z, S2 xx xy xz yy yz zz of rint((p - p_id) * 2^12)
  std::vector<float> box;       // 6 per facet: min x y z, max x y z
  std::vector<double> plane;    // 7 per facet: centroid, unit normal, rms in metres (filled by planes())
  std::vector<uint8_t> planar;  // per facet: rms <= max_rms and a normal that exists
  // the planes from the integers (pcp_facet_plane_host); root(id, a) = coordinate a of map point id
  template <typename Root>
  void planes(Root root, double max_rms) {
    plane.assign(7 * ids.size(), 0.0);
    planar.assign(ids.size(), 0);
    for (size_t r = 0; r < ids.size(); ++r) {
      const float at[3] = {root(ids[r], 0), root(ids[r], 1), root(ids[r], 2)};
      if (pcp_facet_plane_host(at, rows.data() + 10 * r, plane.data() + 7 * r) != PCP_OK)
        throw std::runtime_error(std::string("pcp_hip: ") + pcp_last_error(nullptr));
      const double *pl = plane.data() + 7 * r;
      planar[r] = pl[6] <= max_rms && (pl[3] != 0.0 || pl[4] != 0.0 || pl[5] != 0.0) ? 1 : 0;
    }
  }
};

struct CrackMap {
  int64_t contributors = 0, credited = 0;  // summed over the added keyframes
  int64_t crack_points = 0;
  std::vector<float> width_mean, width_best;  // metres; 0 without a credited keyframe
  std::vector<uint32_t> views;
  std::vector<int32_t> label;      // the crack's id (the lowest input index of its points), -1: no crack point
  std::vector<int32_t> ids;
  std::vector<int64_t> stats;      // 5 per crack: points, sum_w, min_w, max_w (quanta of 2^-20 m), centre_points
  std::vector<float> box;          // 6 per crack: min x y z, max x y z
};

// The lengths of the map's cracks (pcp_hip.h, "crack lengths on the map"): one row per crack, the rows and order of CrackMap,
// and per map point its arc position along its crack
struct CrackLengths {
  std::vector<uint64_t> pos;       // units of 2^-20 m from the crack's end a; 2^64 - 1: no crack point
  std::vector<int32_t> ids;
  std::vector<int64_t> rows;       // 7 per crack: end_a, end_b, length_q, hops, path_sum_w, path_min_w, path_max_w
  std::vector<int64_t> offsets;    // cracks + 1: crack k's polyline is path[offsets[k] .. offsets[k + 1])
  std::vector<int32_t> path;       // input indices, from end a to end b
  double seconds = 0.0;            // wall time of the stage (the call and its fetches)
};

// The directions of the map's cracks (pcp_hip.h, "crack directions on the map"): per map point the tangent of its crack there,
// per crack -- the rows and order of CrackMap -- the sums the axis is taken from, and the axis (pcp_crack_axis_host)
struct CrackDirections {
  std::vector<float> tangent;      // 3 per point: unit, the largest component positive; zeros: none (fewer than two links)
  std::vector<float> anisotropy;   // l1 / trace of the point's link covariance: 1 on a line; 0: none
  std::vector<int32_t> links;      // the point's links
  std::vector<int32_t> ids;
  std::vector<int64_t> rows;       // 20 per crack: (lo, hi) of the summed links, S1 x y z, S2 xx xy xz yy yz zz
  std::vector<double> axis;        // 5 per crack: ordered links, the unit axis (zeros: none), its anisotropy
  double seconds = 0.0;            // wall time of the stage (the call, its fetch and the axes)
};

// The skeletons of the map's cracks (pcp_hip.h, "crack skeletons on the map"): the level-set diagram of every crack -- nodes,
// edges and one summary row per crack, the rows and order of CrackMap -- and per map point the id of its node.  The library
// returns integers only; the metres are host arithmetic on them, here in one place.
struct CrackSkeleton {
  std::vector<int32_t> node;       // the id of the point's node (the lowest input index among its points); -1: no crack point
  std::vector<int32_t> ids;        // per node, ascending
  std::vector<int64_t> nodes;      // 10 per node: crack_row, band, points, sum_w, min_w, max_w, sum_qx, sum_qy, sum_qz, degree
  std::vector<int64_t> edges;      // 3 per edge: u (the node row in the lower band), v, links; ascending by (u, v)
  std::vector<int64_t> cracks;     // 6 per crack: nodes, edges, ends, junctions, loops, max_degree
  double seconds = 0.0;            // wall time of the stage (the call and its fetches)
  // a node's centroid on one axis (0..2), metres
  double centroid(size_t node_row, int axis) const {
    const int64_t *row = nodes.data() + 10 * node_row;
    return (static_cast<double>(row[6 + axis]) / static_cast<double>(row[2])) * (1.0 / 1048576.0);
  }
  // the distance of an edge's two centroids, metres
  double edgeLength(size_t edge_row) const {
    const size_t u = static_cast<size_t>(edges[3 * edge_row]), v = static_cast<size_t>(edges[3 * edge_row + 1]);
    const double dx = centroid(v, 0) - centroid(u, 0), dy = centroid(v, 1) - centroid(u, 1), dz = centroid(v, 2) - centroid(u, 2);
    return std::sqrt((dx * dx + dy * dy) + dz * dz);
  }
  // per crack the sum of its edges' lengths in row order, metres
  std::vector<double> skeletonLengths() const {
    std::vector<double> length(cracks.size() / 6, 0.0);
    for (size_t e = 0; e < edges.size() / 3; ++e) length[static_cast<size_t>(nodes[10 * static_cast<size_t>(edges[3 * e])])] += edgeLength(e);
    return length;
  }
};

// The branches of the map's cracks (pcp_hip.h, "crack branches on the map"): the skeleton cut at its junctions, short spurs
// pruned, one row per branch, and per map point the id of its branch.  The library returns integers; the lengths are
// pcp_crack_branch_lengths_host's, the axes pcp_crack_axis_host's.
struct CrackBranches {
  std::vector<int32_t> branch;       // the id of the point's branch; -1: no crack point, -2: a kept junction, -3: pruned
  std::vector<int32_t> ids;          // per branch, ascending
  std::vector<int64_t> rows;         // 15 per branch: crack_row nodes edges_inside attachments junction_u junction_v points sum_w
                                     // min_w max_w pos_min pos_max sum_qx sum_qy sum_qz
  std::vector<int64_t> moments;      // 20 per branch: (lo, hi) of the links inside it
  std::vector<int32_t> edge_branch;  // per edge of the skeleton: the branch row; -1: a bridge, -2: an edge with a pruned end
  std::vector<int64_t> cracks;       // 7 per crack: branches bridges junctions_kept ends_kept pruned_branches pruned_nodes pruned_points
  std::vector<double> axis;          // 5 per branch: ordered links, the unit axis (zeros: none), its anisotropy
  std::vector<double> length_m;      // per branch
  std::vector<double> kept_length_m; // per crack
  float step = 0.0f, prune = 0.0f;   // as the stage took them
  int64_t pruned_branches = 0;
  double seconds = 0.0;              // wall time of the stage (the call, its fetches, the lengths and the axes)
  // a branch's centroid on one axis (0..2), metres
  double centroid(size_t row, int axis_) const {
    return (static_cast<double>(rows[15 * row + 12 + static_cast<size_t>(axis_)]) / static_cast<double>(rows[15 * row + 6])) * (1.0 / 1048576.0);
  }
  // the mean fused width of a branch's points, metres
  double meanWidth(size_t row) const { return (static_cast<double>(rows[15 * row + 7]) / static_cast<double>(rows[15 * row + 6])) * (1.0 / 1048576.0); }
};

class Device {
 public:
  explicit Device(int ordinal = 0) {
    if (pcp_create(ordinal, &ctx_) != PCP_OK) throw std::runtime_error(std::string("pcp_hip: ") + pcp_last_error(nullptr));
  }
  ~Device() { pcp_destroy(ctx_); }
  Device(const Device &) = delete;
  Device &operator=(const Device &) = delete;
  pcp_context *get() const { return ctx_; }
  static void growText(std::vector<char> &text, int64_t rows, int32_t kind) {
    const size_t need = static_cast<size_t>(rows) * static_cast<size_t>(pcp_ascii_row_bound(kind));
    if (text.size() < need) text.resize(need);
  }
  void check(int rc) const {
    if (rc != PCP_OK) throw std::runtime_error(std::string("pcp_hip: ") + pcp_last_error(ctx_));
  }

  // `cloud` of the reference: pcl::PointCloud<pcl::PointXYZI>::points.data(), stride sizeof(pcl::PointXYZI) == 32
  void uploadCloudAoS(const void *points, int64_t n, int64_t stride_bytes) { check(pcp_upload_cloud_aos(ctx_, points, n, stride_bytes)); }
  void uploadCloud(const float *x, const float *y, const float *z, int64_t n) { check(pcp_upload_cloud(ctx_, x, y, z, n)); }
  // pcl::PointXYZI::intensity of every point (the NID stage bins it, nid_cost.hpp:55-56)
  void uploadIntensity(const float *intensity, int64_t n) { check(pcp_upload_intensity(ctx_, intensity, n)); }
  int64_t cloudSize() const { return pcp_cloud_size(ctx_); }

  // K_camera_coefficients / D_camera (PointCloudProcessor.cpp:57-62) + ViewCulling image size (:525)
  void setCamera(const pcp_camera &cam, const pcp_cull_params *cull = nullptr) { check(pcp_set_camera(ctx_, &cam, cull)); }
  // selectedKeyframes' poses; T_camera_lidar_optimized when NID / manual guess ran (:504-519)
  void setKeyframes(const std::vector<pcp_pose> &poses, const double *T_opt = nullptr, int T_opt_stride = 0) {
    check(pcp_set_frames(ctx_, poses.data(), static_cast<int32_t>(poses.size()), T_opt, T_opt_stride));
  }
  // generateColorMap's cvtColor(BGR2HSV) -> S, V scaling -> cvtColor(HSV2BGR) (PointCloudProcessor.cpp:722-741) done
  // by the library while it packs an uploaded image: enable it and hand over cv::imread's pixels, or leave it off
  // and hand over `adjusted_image`
  void setImageAdjust(bool enable, float saturation_scale = 1.0f, float brightness_scale = 1.0f) {
    check(pcp_set_image_adjust(ctx_, enable ? 1 : 0, saturation_scale, brightness_scale));
  }
  // scripts/image_color_balance_autonomous.py / image_color_balance.py (apply_clahe, adjust_gamma) run over the keyframe folder,
  // done by the library on every image uploaded from now on, before setImageAdjust's round trip; nullptr: off
  void setImageBalance(const pcp_balance_params *params) { check(pcp_set_image_balance(ctx_, params)); }
  // cv::Mat rgb (CV_8UC3; after the HSV round trip unless setImageAdjust(true)): data, step
  void uploadImage(int keyframe, const uint8_t *bgr, int64_t step) { check(pcp_upload_image(ctx_, keyframe, bgr, step)); }
  // decoded frames in pinned memory: queues the copy only; the buffer must outlive the next synchronising call
  void uploadImageAsync(int keyframe, const uint8_t *bgr, int64_t step) { check(pcp_upload_image_async(ctx_, keyframe, bgr, step)); }
  // cv::imread of a keyframe JPEG left to the device: `coeffs.blob` is jpeg_coefficients' blob (host/image_io.hpp JpegCoeffs;
  // pcp_jpeg_header).  Same rules as uploadImage / uploadImageAsync.
  template <class Coeffs>
  void uploadImageJpeg(int keyframe, const Coeffs &coeffs) {
    check(pcp_upload_image_jpeg(ctx_, keyframe, coeffs.blob.data(), static_cast<int64_t>(coeffs.blob.size())));
  }
  template <class Coeffs>
  void uploadImageJpegAsync(int keyframe, const Coeffs &coeffs) {
    check(pcp_upload_image_jpeg_async(ctx_, keyframe, coeffs.blob.data(), static_cast<int64_t>(coeffs.blob.size())));
  }
  // cv::Mat grayImg (CV_8UC1)
  void uploadMask(int keyframe, const uint8_t *gray, int64_t step) { check(pcp_upload_mask(ctx_, keyframe, gray, step)); }

  // ---- device PCD writer: the rows of the ASCII files as text (pcp_hip.h, "device PCD writer").  `text` is the caller's
  // buffer, grown to the window's bound when it is smaller and never shrunk: a loop over windows reuses it. ----
  struct TextWindow {
    int64_t rows = 0, bytes = 0;
  };
  // n rows held on the host (pcp_ascii_rows): the writeASCII_* sites whose arrays are host arrays
  int64_t asciiRows(int32_t kind, int64_t n, const float *f, const uint8_t *rgb, const uint16_t *mask, std::vector<char> &text) const {
    growText(text, n, kind);
    int64_t bytes = 0;
    check(pcp_ascii_rows(ctx_, kind, n, f, rgb, mask, static_cast<int64_t>(text.size()), text.data(), &bytes));
    return bytes;
  }
  // rows [first_row, first_row + max_rows) of removePointsWithNoColor's survivors (pcp_colour_compact_ascii)
  TextWindow colourCompactAscii(bool with_label, int64_t first_row, int64_t max_rows, std::vector<char> &text) const {
    growText(text, max_rows, with_label ? PCP_ROWS_XYZRGBMASK : PCP_ROWS_XYZRGB);
    TextWindow w;
    check(pcp_colour_compact_ascii(ctx_, with_label ? 1 : 0, first_row, max_rows, static_cast<int64_t>(text.size()), text.data(), &w.rows,
                                   &w.bytes));
    return w;
  }
  // rows [first_row, first_row + max_rows) of the latest smoothing result (pcp_mls_fetch_ascii)
  TextWindow mlsFetchAscii(int64_t first_row, int64_t max_rows, std::vector<char> &text) const {
    growText(text, max_rows, PCP_ROWS_POINTNORMAL);
    TextWindow w;
    check(pcp_mls_fetch_ascii(ctx_, first_row, max_rows, static_cast<int64_t>(text.size()), text.data(), &w.rows, &w.bytes));
    return w;
  }

  // ---- voxel-grid output: what pcl::VoxelGrid at `leaf` (voxelgrid_sampling, frame_cpu.cpp:360-451) makes of the coloured
  // cloud, accumulated on the device over any number of colour results (pcp_voxel_reduce_*; DESIGN.md "Voxel-grid output") ----
  void voxelReduceBegin(float leaf, int64_t initial_slots = 0) { check(pcp_voxel_reduce_begin(ctx_, leaf, initial_slots)); }
  int64_t voxelReduceAdd() {  // the coloured rows of the current colour result; returns their number
    int64_t rows = 0;
    check(pcp_voxel_reduce_add(ctx_, &rows));
    return rows;
  }
  int64_t voxelReduceFinish() {
    int64_t voxels = 0;
    check(pcp_voxel_reduce_finish(ctx_, &voxels));
    return voxels;
  }
  VoxelCloud voxelReduceFetch(bool with_label) {  // the whole finished result
    VoxelCloud v;
    const size_t m = static_cast<size_t>(voxelReduceFinish());
    v.xyz.resize(3 * m);
    v.rgb.resize(3 * m);
    v.label.resize(with_label ? m : 0);
    v.count.resize(m);
    int64_t rows = 0;
    check(pcp_voxel_reduce_fetch(ctx_, 0, static_cast<int64_t>(m), v.xyz.data(), v.rgb.data(), with_label ? v.label.data() : nullptr,
                                 v.count.data(), &rows));
    return v;
  }
  std::vector<int64_t> voxelReduceStats() const {  // rows, voxels, slots, doublings, wavefront partials, global adds
    std::vector<int64_t> s(6);
    check(pcp_voxel_reduce_stats(ctx_, s.data()));
    return s;
  }
  void voxelReduceEnd() { check(pcp_voxel_reduce_end(ctx_)); }

  // ---- orthographic maps: one metric picture of the coloured cloud, accumulated on the device over any number of colour
  // results (pcp_ortho_*; DESIGN.md "Orthographic maps") ----
  void orthoBegin(const pcp_ortho_frame &frame) {
    check(pcp_ortho_begin(ctx_, &frame));
    ortho_frame_ = frame;  // (only of a begin the library took: a refused one leaves the live map, and its frame, as they were)
  }
  // the same accumulator under a cylinder's frame, unrolled along its arc (pcp_ortho_begin_cyl; DESIGN.md "Cylindrical facets"):
  // the adds, orthoFetch, orthoStats and orthoEnd work on either kind; orthoTexture is refused on this one, orthoTextureCyl is its call
  void orthoBeginCyl(const pcp_cyl_frame &frame) {
    check(pcp_ortho_begin_cyl(ctx_, &frame));
    ortho_frame_ = pcp_ortho_frame{};  // (orthoFetch sizes its layers by the raster of the last begin the library took)
    ortho_frame_.gsd = frame.gsd;
    ortho_frame_.width = frame.width;
    ortho_frame_.height = frame.height;
  }
  int64_t orthoAdd(int64_t index_base = 0) {  // the coloured rows of the current colour result; returns the contributors
    int64_t rows = 0;
    check(pcp_ortho_add(ctx_, index_base, &rows));
    return rows;
  }
  int64_t orthoAddFacet(int32_t facet_id, int64_t index_base = 0) {  // orthoAdd restricted to the rows of one facet of the last facets()
    int64_t rows = 0;
    check(pcp_ortho_add_facet(ctx_, facet_id, index_base, &rows));
    return rows;
  }
  int64_t orthoAddPacked(const uint32_t *rgba, int64_t index_base = 0) {  // cloudSize() words r | g<<8 | b<<16 | has<<24
    int64_t rows = 0;
    check(pcp_ortho_add_packed(ctx_, rgba, index_base, &rows));
    return rows;
  }
  // finish (fill_radius_px > 0: empty pixels take their nearest occupied pixel within it) and fetch every layer
  // (the layers are sized by the frame of the last orthoBegin that succeeded on this Device: the live map's)
  OrthoMap orthoFetch(int32_t fill_radius_px, bool with_label) {
    OrthoMap m;
    const pcp_ortho_frame &frame = m.frame = ortho_frame_;
    check(pcp_ortho_finish(ctx_, fill_radius_px, &m.occupied, &m.filled));
    m.contributors = orthoStats()[0];
    const size_t px = static_cast<size_t>(frame.width) * static_cast<size_t>(frame.height);
    m.index.resize(px);
    m.depth.resize(px);
    m.rgb.resize(3 * px);
    m.label.resize(with_label ? px : 0);
    m.status.resize(px);
    m.source.resize(px);
    check(pcp_ortho_fetch(ctx_, m.index.data(), m.depth.data(), m.rgb.data(), with_label ? m.label.data() : nullptr, m.status.data(),
                          m.source.data()));
    return m;
  }
  std::vector<int64_t> orthoStats() const {  // contributors, atomics issued, occupied, filled, adds, pixels
    std::vector<int64_t> s(6);
    check(pcp_ortho_stats(ctx_, s.data()));
    return s;
  }
  void orthoEnd() { check(pcp_ortho_end(ctx_)); }
  // The surface defects of the live, finished map (pcp_ortho_defects): the counts; the layers and the table stay on the device
  // for orthoDefectsFetch, which sizes them by the frame of the last orthoBegin that succeeded on this Device.
  OrthoDefects orthoDefects(const pcp_ortho_defect_params &p) {
    OrthoDefects d;
    check(pcp_ortho_defects(ctx_, &p, d.counts));
    return d;
  }
  void orthoDefectsFetch(OrthoDefects &d) {
    const size_t px = static_cast<size_t>(ortho_frame_.width) * static_cast<size_t>(ortho_frame_.height);
    d.dev.resize(px);
    d.cls.resize(px);
    d.region.resize(px);
    check(pcp_ortho_defects_fetch(ctx_, d.dev.data(), d.cls.data(), d.region.data()));
    int64_t rows = 0;
    check(pcp_ortho_defects_table(ctx_, 0, int64_t(1) << 40, nullptr, &rows));
    d.rows.assign(static_cast<size_t>(16 * rows), 0);
    if (rows) check(pcp_ortho_defects_table(ctx_, 0, rows, d.rows.data(), &rows));
  }
  // The orthophoto of the live, finished map (pcp_ortho_texture; DESIGN.md "Orthophotos"): p.scale fine pixels per ortho pixel
  // and axis over the rectangle p names (w == 0 && h == 0: the whole raster), coloured straight from the keyframe images under
  // the depth maps the context holds.  (Sized by the frame of the last orthoBegin that succeeded on this Device; parameters the
  // library refuses get no layers and its refusal.)
  OrthoPhoto orthoTexture(const pcp_ortho_texture_params &p) { return orthoTextureBy(pcp_ortho_texture, p); }
  // the same of a cylinder's unrolled map (pcp_ortho_texture_cyl; DESIGN.md "Orthophotos of unrolled maps"): after orthoBeginCyl
  OrthoPhoto orthoTextureCyl(const pcp_ortho_texture_params &p) { return orthoTextureBy(pcp_ortho_texture_cyl, p); }
  OrthoPhoto orthoTextureBy(decltype(&pcp_ortho_texture) call, const pcp_ortho_texture_params &p) {
    OrthoPhoto ph;
    const int64_t w = (p.w == 0 && p.h == 0) ? ortho_frame_.width : p.w, h = (p.w == 0 && p.h == 0) ? ortho_frame_.height : p.h;
    const int64_t k = p.scale;
    if (k >= 1 && k <= 16 && w >= 1 && h >= 1 && w * h * k * k <= (int64_t(1) << 28)) {
      ph.width = static_cast<int32_t>(w * k);
      ph.height = static_cast<int32_t>(h * k);
    }
    const size_t px = static_cast<size_t>(ph.width) * static_cast<size_t>(ph.height);
    ph.rgb.resize(3 * px);
    ph.mask.resize(px);
    ph.status.resize(px);
    ph.view.resize(px);
    ph.count.resize(px);
    int64_t counts[4] = {0, 0, 0, 0};
    check(call(ctx_, &p, ph.rgb.data(), ph.mask.data(), ph.status.data(), ph.view.data(), ph.count.data(), counts));
    ph.surface = counts[0];
    ph.textured = counts[1];
    ph.unseen = counts[2];
    ph.skipped_pairs = counts[3];
    return ph;
  }
  // the frame that looks straight at n rows (xyz interleaved; has nullable) from the side of `viewer` (3 doubles, nullable)
  static pcp_ortho_frame orthoFitFrame(int64_t n, const float *xyz, const uint8_t *has, const double *viewer, float gsd) {
    pcp_ortho_frame f{};
    if (pcp_ortho_fit_frame_host(n, xyz, has, viewer, gsd, &f) != PCP_OK)
      throw std::runtime_error(std::string("pcp_hip: ") + pcp_last_error(nullptr));
    return f;
  }
  // the cylinder of the rows that have a valid normal (3 floats per row) and the frame that unrolls them (pcp_cyl_fit_host);
  // stats (nullable, 8 doubles): rows, rms, least and greatest rho - R, occupied arc, the normals' three eigenvalues.  false: the
  // rows are no cylinder this fit can give (PCP_ERR_RANGE; *why, nullable, receives the message); anything else throws
  static bool orthoFitCylinder(int64_t n, const float *xyz, const float *normal, const uint8_t *has, const double *viewer, float gsd,
                               pcp_cyl_frame *out, double *stats = nullptr, std::string *why = nullptr) {
    const int rc = pcp_cyl_fit_host(n, xyz, normal, has, viewer, gsd, out, stats);
    if (rc == PCP_OK) return true;
    if (rc != PCP_ERR_RANGE) throw std::runtime_error(std::string("pcp_hip: ") + pcp_last_error(nullptr));
    if (why) *why = pcp_last_error(nullptr);
    return false;
  }

  // ---- geometry maps: a normal per point of the uploaded map, once per upload (pcp_estimate_normals; what
  // generate_norm_masks estimates per keyframe with Open3D, scripts/genNormAndDistanceMask.py:200-231); returns the valid points
  int64_t estimateNormals(float radius) {
    int64_t valid = 0;
    check(pcp_estimate_normals(ctx_, radius, &valid, nullptr));
    return valid;
  }

  // ---- map comparison: the uploaded map against `n_base` interleaved xyz rows of an earlier survey under the live normals
  // (pcp_compare_set_base, pcp_compare and its fetch; the base is dropped again); needs estimateNormals
  // ---- map registration: the base that pcp_compare_set_base left, brought onto the uploaded map under the live normals
  // (pcp_compare_register); needs estimateNormals and a base
  Registration registerBase(const pcp_register_params &p) {
    Registration r;
    r.log.assign(5 * static_cast<size_t>(p.max_iterations > 0 ? p.max_iterations : 1), 0.0);
    int32_t st[2] = {0, 0};
    check(pcp_compare_register(ctx_, &p, nullptr, r.T, r.log.data(), st));
    r.status = st[0];
    r.iterations = st[1];
    r.log.resize(5 * static_cast<size_t>(st[1]));
    if (st[1] > 0) {
      const double *last = r.log.data() + 5 * static_cast<size_t>(st[1] - 1);
      r.pairs = static_cast<int64_t>(last[0]);
      r.rms = last[1];
      r.dof = static_cast<int32_t>(last[2]);
    }
    return r;
  }

  // ---- coarse registration: the base that pcp_compare_set_base left, brought near the uploaded map from an arbitrary pose
  // under the live normals, its own normals estimated on the device (pcp_compare_register_coarse); registerBase finishes it
  struct CoarseRegistration {
    int64_t report[16] = {0};  // CG8: keypoints, valid descriptors, correspondences, hypotheses, inliers, status, the winner
    double T[16] = {0};
    int32_t status() const { return static_cast<int32_t>(report[11]); }  // 0 found, 2 too few inliers (T as it was)
  };
  CoarseRegistration registerBaseCoarse(const pcp_coarse_params &p) {
    CoarseRegistration r;
    check(pcp_compare_register_coarse(ctx_, &p, nullptr, nullptr, r.report, r.T, nullptr));
    return r;
  }

  // (reg: the base is registered onto the map first, *registration filled)
  MapComparison compareMap(const pcp_compare_params &p, const float *base_xyz, int64_t n_base, const pcp_register_params *reg = nullptr,
                           Registration *registration = nullptr) {
    MapComparison m;
    const size_t n = static_cast<size_t>(cloudSize());
    m.distance.resize(n);
    m.lod.resize(n);
    m.status.resize(n);
    check(pcp_compare_set_base(ctx_, base_xyz, n_base, 12));
    struct End {  // also on the way out of an exception
      pcp_context *c;
      ~End() { (void)pcp_compare_end(c); }
    } end{ctx_};
    if (reg) {
      Registration r = registerBase(*reg);
      if (registration) *registration = std::move(r);
    }
    check(pcp_compare(ctx_, &p, nullptr, m.stats));
    check(pcp_compare_fetch(ctx_, m.distance.data(), m.lod.data(), m.status.data(), nullptr, nullptr));
    return m;
  }

  // ---- planar facets: the faces of the uploaded map under the live normals (pcp_facets and its fetch); needs estimateNormals
  Facets facets(const pcp_facet_params &p) {
    Facets f;
    f.label.resize(static_cast<size_t>(cloudSize()));
    int64_t rows = 0, got = 0;
    check(pcp_facets(ctx_, &p, f.label.data(), &f.facet_points, &f.components, &rows));
    f.ids.resize(static_cast<size_t>(rows));
    f.rows.resize(10 * static_cast<size_t>(rows));
    f.box.resize(6 * static_cast<size_t>(rows));
    check(pcp_facets_fetch(ctx_, 0, rows, f.ids.data(), f.rows.data(), f.box.data(), &got));
    if (got != rows) throw std::runtime_error("pcp_hip: pcp_facets_fetch returned " + std::to_string(got) + " of " + std::to_string(rows) + " rows");
    return f;
  }

  // ---- mask distance maps: the squared Euclidean distance transform of the uploaded masks of keyframes first .. first +
  // count - 1 and the nearest background pixel (a mask byte above `threshold` is foreground), in one call; what preprocess()
  // computes per mask with cv2.threshold and scipy's distance_transform_edt (scripts/genNormAndDistanceMask.py:167-169)
  MaskDistance maskDistance(int first, int count, int32_t width, int32_t height, int threshold = 0, bool with_nearest = true) {
    MaskDistance d;
    d.width = width;
    d.height = height;
    d.count = count;
    const size_t px = static_cast<size_t>(width) * static_cast<size_t>(height) * static_cast<size_t>(count > 0 ? count : 0);
    d.d2.resize(px);
    d.nearest.resize(with_nearest ? px : 0);
    check(pcp_mask_edt_frames(ctx_, first, count, threshold, d.d2.data(), with_nearest ? d.nearest.data() : nullptr));
    return d;
  }

  // ---- device PCD reader: the x y z intensity floats of a window of PCD ASCII rows (pcp_hip.h, "device PCD reader") ----
  struct ParsedRows {
    int64_t rows = 0, consumed = 0, bad_row = -1;
  };
  // text[0, bytes): rows of `columns` tokens, x y z intensity at columns col[0..3] (col[3] = -1: none); the arrays hold
  // max_rows floats (pcp_ascii_parse).  A bad row is not an exception: bad_row names it and the rows in front of it are in.
  ParsedRows parseAscii(const char *text, int64_t bytes, int32_t columns, const int32_t col[4], bool final_window, int64_t max_rows,
                        float *x, float *y, float *z, float *intensity) const {
    ParsedRows r;
    check(pcp_ascii_parse(ctx_, text, bytes, columns, col, final_window ? 1 : 0, max_rows, x, y, z, intensity, &r.rows, &r.consumed,
                          &r.bad_row));
    return r;
  }

 private:
  pcp_context *ctx_ = nullptr;
  pcp_ortho_frame ortho_frame_{};  // of the live orthographic map
};

// vlcal::ViewCulling with the z-buffer routine (view_culling.cpp:52-174)
class ViewCulling {
 public:
  explicit ViewCulling(Device &dev) : dev_(dev) {}
  // indices of the kept points in input order (what `sample(points, point_indices)` consumes)
  std::vector<int32_t> cull(int keyframe) const {
    std::vector<uint8_t> keep(static_cast<size_t>(dev_.cloudSize()));
    int64_t kept = 0;
    dev_.check(pcp_cull_frame(dev_.get(), keyframe, keep.data(), &kept, nullptr));
    std::vector<int32_t> idx;
    idx.reserve(static_cast<size_t>(kept));
    for (size_t i = 0; i < keep.size(); ++i)
      if (keep[i]) idx.push_back(static_cast<int32_t>(i));
    return idx;
  }
  // the images generate_distance_masks / generate_norm_masks scatter from the culled cloud of one keyframe
  // (scripts/genNormAndDistanceMask.py:200-266), reduced on the device: the nearest kept point wins a pixel.  with_normals
  // needs Device::estimateNormals on the uploaded cloud.
  GeometryMaps geometryMaps(int keyframe, int32_t width, int32_t height, bool with_normals) const {
    GeometryMaps g;
    g.width = width;
    g.height = height;
    const size_t px = static_cast<size_t>(width) * static_cast<size_t>(height);
    g.index.resize(px);
    g.range.resize(px);
    g.xyz_cam.resize(3 * px);
    g.normal_cam.resize(with_normals ? 3 * px : 0);
    dev_.check(pcp_frame_geometry(dev_.get(), keyframe, g.index.data(), g.range.data(), g.xyz_cam.data(),
                                  with_normals ? g.normal_cam.data() : nullptr, &g.pixels));
    return g;
  }
  // what compute_skeleton_edge_pts measures at hand-picked skeleton points (scripts/genNormAndDistanceMask.py:396-478), at
  // every foreground pixel of the keyframe's uploaded mask: edge points along the EDT direction, the local plane of the
  // position image within +-plane_radius pixels, and the 3-D width between the edge rays on it
  CrackWidth crackWidth(int keyframe, int32_t width, int32_t height, int threshold = 0, int plane_radius = 150,
                        bool with_plane = false) const {
    CrackWidth c;
    c.width = width;
    c.height = height;
    const size_t px = static_cast<size_t>(width) * static_cast<size_t>(height);
    c.flags.resize(px);
    c.edges.resize(4 * px);
    c.width_m.resize(px);
    c.points.resize(6 * px);
    c.plane.resize(with_plane ? 4 * px : 0);
    const pcp_crack_params prm{threshold, plane_radius};
    dev_.check(pcp_crack_width(dev_.get(), keyframe, &prm, c.flags.data(), c.edges.data(), nullptr, c.width_m.data(), c.points.data(),
                               with_plane ? c.plane.data() : nullptr, nullptr, &c.sites, &c.widths));
    return c;
  }
  // crackWidth's widths of the given keyframes brought back to the `points` map points that see them, and the connected
  // components of the points with min_views credited keyframes or more under the link radius: what the script's result file
  // (scripts/genNormAndDistanceMask.py:476-478) lists per hand-picked pixel, for the whole map and with the cracks told apart
  // lengths (nullable): also the cracks' lengths, ends and centrelines for the same min_views and link radius
  // skeleton (nullable): also the cracks' skeletons for them and the band width skeleton_step (metres; 0: 2 * link_radius)
  // directions (nullable): also the cracks' directions for the same min_views and link radius
  // branches (nullable): also the cracks' branches for them, skeleton_step and the bound prune (metres; below 0: twice the band width)
  CrackMap crackMap(const std::vector<int> &keyframes, int64_t points, int threshold = 0, int plane_radius = 150, int min_views = 1,
                    float link_radius = 0.02f, CrackLengths *lengths = nullptr, CrackSkeleton *skeleton = nullptr,
                    float skeleton_step = 0.0f, CrackDirections *directions = nullptr, CrackBranches *branches = nullptr,
                    float prune = -1.0f) const {
    CrackMap m;
    dev_.check(pcp_crack_fuse_begin(dev_.get()));
    try {
      const pcp_crack_params prm{threshold, plane_radius};
      for (int k : keyframes) {
        int64_t listed = 0, credited = 0;
        dev_.check(pcp_crack_fuse_add(dev_.get(), k, &prm, &listed, &credited));
        m.contributors += listed;
        m.credited += credited;
      }
      const size_t n = static_cast<size_t>(points);
      m.width_mean.resize(n);
      m.width_best.resize(n);
      m.views.resize(n);
      m.label.resize(n);
      dev_.check(pcp_crack_fuse_fetch(dev_.get(), m.width_mean.data(), m.width_best.data(), nullptr, m.views.data(), nullptr, nullptr,
                                      nullptr, nullptr, nullptr));
      const pcp_crack_link_params link{min_views, link_radius};
      int64_t rows = 0, got = 0;
      dev_.check(pcp_crack_components(dev_.get(), &link, m.label.data(), &m.crack_points, &rows));
      m.ids.resize(static_cast<size_t>(rows));
      m.stats.resize(5 * static_cast<size_t>(rows));
      m.box.resize(6 * static_cast<size_t>(rows));
      dev_.check(pcp_crack_components_fetch(dev_.get(), 0, rows, m.ids.data(), m.stats.data(), m.box.data(), &got));
      if (directions) *directions = crackDirections(points, min_views, link_radius);  // (it leaves the same component table)
      if (lengths) *lengths = crackLengths(points, min_views, link_radius);
      if (skeleton) *skeleton = crackSkeleton(points, min_views, link_radius, skeleton_step);
      if (branches) *branches = crackBranches(points, min_views, link_radius, skeleton_step, prune);  // (it leaves the same three tables)
    } catch (...) {
      (void)pcp_crack_fuse_end(dev_.get());
      throw;
    }
    dev_.check(pcp_crack_fuse_end(dev_.get()));
    return m;
  }
  // The geodesic length, the two ends and the ordered polyline of every crack of the live accumulation (between
  // pcp_crack_fuse_begin and _end; crackMap runs it when asked), and every point's arc position
  CrackLengths crackLengths(int64_t points, int min_views = 1, float link_radius = 0.02f) const {
    CrackLengths c;
    const auto t0 = std::chrono::steady_clock::now();
    c.pos.resize(static_cast<size_t>(points));
    const pcp_crack_link_params link{min_views, link_radius};
    int64_t rows = 0, entries = 0, got = 0;
    dev_.check(pcp_crack_lengths(dev_.get(), &link, c.pos.data(), &rows, &entries));
    c.ids.resize(static_cast<size_t>(rows));
    c.rows.resize(7 * static_cast<size_t>(rows));
    c.offsets.assign(static_cast<size_t>(rows) + 1, 0);
    c.path.resize(static_cast<size_t>(entries));
    dev_.check(pcp_crack_lengths_fetch(dev_.get(), 0, rows, c.ids.data(), c.rows.data(), c.offsets.data(), &got));
    dev_.check(pcp_crack_paths_fetch(dev_.get(), 0, entries, c.path.data(), &got));
    c.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return c;
  }
  // Which way every crack of the live accumulation runs (between pcp_crack_fuse_begin and _end; crackMap runs it when asked):
  // a tangent per crack point and an axis per crack, where scripts/evalSkeletonDirection.py blurs one keyframe's 2-D skeleton
  CrackDirections crackDirections(int64_t points, int min_views = 1, float link_radius = 0.02f) const {
    CrackDirections c;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = static_cast<size_t>(points);
    c.tangent.resize(3 * n);
    c.anisotropy.resize(n);
    c.links.resize(n);
    const pcp_crack_link_params link{min_views, link_radius};
    int64_t crack_points = 0, rows = 0, got = 0;
    dev_.check(pcp_crack_directions(dev_.get(), &link, c.tangent.data(), c.anisotropy.data(), c.links.data(), nullptr, &crack_points, &rows));
    c.ids.resize(static_cast<size_t>(rows));
    c.rows.resize(20 * static_cast<size_t>(rows));
    c.axis.assign(5 * static_cast<size_t>(rows), 0.0);
    dev_.check(pcp_crack_directions_fetch(dev_.get(), 0, rows, c.ids.data(), c.rows.data(), &got));
    for (size_t r = 0; r < static_cast<size_t>(rows); ++r) dev_.check(pcp_crack_axis_host(c.rows.data() + 20 * r, c.axis.data() + 5 * r));
    c.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return c;
  }
  // The level-set diagram of every crack of the live accumulation (between pcp_crack_fuse_begin and _end; crackMap runs it
  // when asked): what pcv.morphology.skeletonize gives the reference's script per keyframe and in 2-D, once and on the map.
  // step: the band width in metres, 0 for 2 * link_radius.
  CrackSkeleton crackSkeleton(int64_t points, int min_views = 1, float link_radius = 0.02f, float step = 0.0f) const {
    CrackSkeleton c;
    const auto t0 = std::chrono::steady_clock::now();
    c.node.resize(static_cast<size_t>(points));
    const pcp_crack_link_params link{min_views, link_radius};
    int64_t nodes = 0, edges = 0, cracks = 0, got = 0;
    dev_.check(pcp_crack_skeleton(dev_.get(), &link, step > 0.0f ? step : 2.0f * link_radius, c.node.data(), &nodes, &edges));
    dev_.check(pcp_crack_skeleton_cracks_fetch(dev_.get(), 0, INT64_MAX / 2, nullptr, &cracks));
    c.ids.resize(static_cast<size_t>(nodes));
    c.nodes.resize(10 * static_cast<size_t>(nodes));
    c.edges.resize(3 * static_cast<size_t>(edges));
    c.cracks.resize(6 * static_cast<size_t>(cracks));
    dev_.check(pcp_crack_skeleton_nodes_fetch(dev_.get(), 0, nodes, c.ids.data(), c.nodes.data(), &got));
    dev_.check(pcp_crack_skeleton_edges_fetch(dev_.get(), 0, edges, c.edges.data(), &got));
    dev_.check(pcp_crack_skeleton_cracks_fetch(dev_.get(), 0, cracks, c.cracks.data(), &got));
    c.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return c;
  }
  // Every crack of the live accumulation arm by arm (between pcp_crack_fuse_begin and _end; crackMap runs it when asked): the
  // diagram of crackSkeleton cut at its junctions, branches with one attachment and nodes * step < prune pruned.  step: the
  // band width in metres, 0 for 2 * link_radius; prune: metres, below 0 for twice the band width.
  CrackBranches crackBranches(int64_t points, int min_views = 1, float link_radius = 0.02f, float step = 0.0f, float prune = -1.0f) const {
    CrackBranches c;
    const auto t0 = std::chrono::steady_clock::now();
    c.branch.resize(static_cast<size_t>(points));
    c.step = step > 0.0f ? step : 2.0f * link_radius;
    c.prune = prune >= 0.0f ? prune : 2.0f * c.step;
    const pcp_crack_link_params link{min_views, link_radius};
    int64_t rows = 0, nodes = 0, edges = 0, cracks = 0, got = 0;
    dev_.check(pcp_crack_branches(dev_.get(), &link, c.step, c.prune, c.branch.data(), &rows, &c.pruned_branches));
    dev_.check(pcp_crack_branch_edges_fetch(dev_.get(), 0, INT64_MAX / 2, nullptr, &edges));
    dev_.check(pcp_crack_branch_cracks_fetch(dev_.get(), 0, INT64_MAX / 2, nullptr, &cracks));
    dev_.check(pcp_crack_skeleton_nodes_fetch(dev_.get(), 0, INT64_MAX / 2, nullptr, nullptr, &nodes));
    const size_t sb = static_cast<size_t>(rows), se = static_cast<size_t>(edges), sc = static_cast<size_t>(cracks);
    c.ids.resize(sb);
    c.rows.resize(15 * sb);
    c.moments.resize(20 * sb);
    c.edge_branch.resize(se);
    c.cracks.resize(7 * sc);
    c.axis.assign(5 * sb, 0.0);
    c.length_m.assign(sb, 0.0);
    c.kept_length_m.assign(sc, 0.0);
    std::vector<int64_t> node_rows(10 * static_cast<size_t>(nodes)), edge_rows(3 * se);
    dev_.check(pcp_crack_branches_fetch(dev_.get(), 0, rows, c.ids.data(), c.rows.data(), c.moments.data(), &got));
    dev_.check(pcp_crack_branch_edges_fetch(dev_.get(), 0, edges, c.edge_branch.data(), &got));
    dev_.check(pcp_crack_branch_cracks_fetch(dev_.get(), 0, cracks, c.cracks.data(), &got));
    dev_.check(pcp_crack_skeleton_nodes_fetch(dev_.get(), 0, nodes, nullptr, node_rows.data(), &got));
    dev_.check(pcp_crack_skeleton_edges_fetch(dev_.get(), 0, edges, edge_rows.data(), &got));
    if (pcp_crack_branch_lengths_host(nodes, node_rows.data(), edges, edge_rows.data(), c.edge_branch.data(), rows, cracks, c.length_m.data(),
                                      c.kept_length_m.data()) != PCP_OK)
      throw std::runtime_error(std::string("pcp_hip: ") + pcp_last_error(nullptr));
    for (size_t r = 0; r < sb; ++r) dev_.check(pcp_crack_axis_host(c.moments.data() + 20 * r, c.axis.data() + 5 * r));
    c.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return c;
  }

 private:
  Device &dev_;
};

struct VisiblePoints {  // one keyframe's coloredCloud / scanInBodyWithRGBandMask
  std::vector<int32_t> index;
  std::vector<uint8_t> rgb;      // 3 per point
  std::vector<uint16_t> mask;    // segmentMask
  std::vector<float> xyz_cam;    // 3 per point, camera frame
  std::vector<float> xyz_world;  // 3 per point, transformPointCloud(c2w)
};

class Colorizer {
 public:
  explicit Colorizer(Device &dev) : dev_(dev) {}
  // rgbCloud.cloudWithSmoothedColor after smoothColors: rgb (3 per input point) and the
  // removePointsWithNoColor keep flag.  How samples are credited back to map points is the camera's cull parameters'
  // match_mode (Device::setCamera): PCP_MATCH_RADIUS reproduces the reference's radiusSearch match-back in full
  // (PointCloudProcessor.cpp:480-482,571-592), every map point within 10 um of a sample receiving it.
  void colorize(std::vector<uint8_t> &rgb, std::vector<uint8_t> &has) const {
    const size_t n = static_cast<size_t>(dev_.cloudSize());
    rgb.resize(3 * n);
    has.resize(n);
    dev_.check(pcp_colorize(dev_.get(), rgb.data(), has.data()));
  }
  // Fused segmentation labels (pcp_set_label_fusion): where the reference appends every keyframe's mask samples to one
  // cloud (PointCloudProcessor.cpp:533-551, the TODO at :938), colorize() then also fuses the masks of each point's top-5
  // views into one label per map point.  Every keyframe needs its mask (Device::uploadMask).  Off by default.
  void setLabelFusion(bool enable) const { dev_.check(pcp_set_label_fusion(dev_.get(), enable ? 1 : 0)); }
  // label, hits (views whose mask is 255) and views (<= 5) of every input point, after colorize() with fusion on;
  // smoothColorsWithLocalRegion leaves them alone
  void labels(std::vector<uint8_t> &label, std::vector<uint8_t> *hits = nullptr, std::vector<uint8_t> *views = nullptr) const {
    const size_t n = static_cast<size_t>(dev_.cloudSize());
    label.resize(n);
    if (hits) hits->resize(n);
    if (views) views->resize(n);
    dev_.check(pcp_colour_labels(dev_.get(), label.data(), hits ? hits->data() : nullptr, views ? views->data() : nullptr));
  }
  // The staged form of colorize(): accumulate() leaves every point's top-5 list on the device (reset, depth pass, colour pass
  // over all keyframes), finalise() turns the lists into rgb / has -- the same bits as colorize().  In between the lists can
  // be read: balanceExposure().
  void accumulate() const {
    const int32_t frames = pcp_frame_count(dev_.get());
    dev_.check(pcp_colour_reset(dev_.get()));
    dev_.check(pcp_depth_pass(dev_.get(), 0, frames));
    dev_.check(pcp_colour_pass(dev_.get(), 0, frames));
  }
  void finalise(std::vector<uint8_t> &rgb, std::vector<uint8_t> &has) const {
    const size_t n = static_cast<size_t>(dev_.cloudSize());
    rgb.resize(3 * n);
    has.resize(n);
    dev_.check(pcp_colour_finalise(dev_.get(), rgb.data(), has.data(), nullptr, nullptr, nullptr, nullptr));
  }
  // One orthographic picture of the colour result colorize() / finalise() left on the device (DESIGN.md "Orthographic maps"):
  // begin, one add under the input indices, finish with the fill radius, fetch, end.  with_label: after a run with label fusion.
  // texture / photo (both or neither): the orthophoto of the finished map under these parameters, before the map ends.
  OrthoMap orthoMap(const pcp_ortho_frame &frame, int32_t fill_radius_px = 0, bool with_label = false,
                    const pcp_ortho_texture_params *texture = nullptr, OrthoPhoto *photo = nullptr) const {
    dev_.orthoBegin(frame);
    struct End {  // also on the way out of an exception
      Device &d;
      ~End() { (void)pcp_ortho_end(d.get()); }
    } end{dev_};
    (void)dev_.orthoAdd(0);
    OrthoMap m = dev_.orthoFetch(fill_radius_px, with_label);
    if (texture && photo) *photo = dev_.orthoTexture(*texture);
    return m;
  }
  // the same result left on the device (for pcp_colour_smooth_local, pcp_colour_compact, pcp_voxel_reduce_add): nothing is fetched
  void finaliseOnDevice() const {
    dev_.check(pcp_colour_finalise(dev_.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  }
  // Exposure gains (DESIGN.md "Exposure gains"; the reference's one hand-set brightness is PointCloudProcessor.cpp:726-729, its
  // pairwise note RGBCloud.hpp:20-25): after accumulate(), the pair statistics of the lists (pcp_view_pair_stats), one gain
  // per keyframe from them (pcp_exposure_gains) and the gains set for finalise() (pcp_set_frame_gains).  Returns the gains.
  // colorize() refuses to run while they are set: clearExposureGains().
  std::vector<double> balanceExposure(double sigma_n = 10.0, double sigma_g = 0.1) const {
    const int32_t frames = pcp_frame_count(dev_.get());
    const size_t cells = static_cast<size_t>(frames) * static_cast<size_t>(frames);
    std::vector<uint64_t> pairs(cells), sums(cells);
    dev_.check(pcp_view_pair_stats(dev_.get(), pairs.data(), sums.data()));
    std::vector<double> gains(static_cast<size_t>(frames), 1.0);
    if (pcp_exposure_gains(frames, pairs.data(), sums.data(), sigma_n, sigma_g, gains.data()) != PCP_OK)
      throw std::runtime_error(std::string("pcp_exposure_gains: ") + pcp_last_error(nullptr));
    dev_.check(pcp_set_frame_gains(dev_.get(), gains.data(), frames));
    return gains;
  }
  void clearExposureGains() const { dev_.check(pcp_set_frame_gains(dev_.get(), nullptr, 0)); }
  // PointCloudProcessor::smoothColorsWithLocalRegion(rgbCloud, radius), PointCloudProcessor.cpp:634-703 (its call
  // smoothColorsWithLocalRegion(rgbCloud, 0.1) is commented out at :597): in place on the result of colorize(); rgb / has
  // (3 + 1 per input point) receive the smoothed colours and the removePointsWithNoColor flag.  Returns the coloured points.
  int64_t smoothColorsWithLocalRegion(float radius, std::vector<uint8_t> &rgb, std::vector<uint8_t> &has) const {
    const size_t n = static_cast<size_t>(dev_.cloudSize());
    int64_t coloured = 0;
    dev_.check(pcp_colour_smooth_local(dev_.get(), radius, &coloured));
    std::vector<uint32_t> words(n);
    dev_.check(pcp_download_result_packed(dev_.get(), words.data()));
    rgb.resize(3 * n);
    has.resize(n);
    for (size_t i = 0; i < n; ++i) {
      const uint32_t v = words[i];
      rgb[3 * i] = static_cast<uint8_t>(v & 0xffu);
      rgb[3 * i + 1] = static_cast<uint8_t>((v >> 8) & 0xffu);
      rgb[3 * i + 2] = static_cast<uint8_t>((v >> 16) & 0xffu);
      has[i] = static_cast<uint8_t>((v >> 24) & 1u);
    }
    return coloured;
  }
  // One cull per keyframe as a rule.  The outputs are sized by the largest keyframe seen so far (a keyframe sees a few
  // per cent of the map; sizing them for the whole cloud meant 33 B x n of zero-filled vectors per call, 1.65 GB at
  // 50 M points -- ADVICE r2); a keyframe that needs more reports its count and is fetched again with room for it.
  VisiblePoints frameVisible(int keyframe) const {
    const size_t n = static_cast<size_t>(dev_.cloudSize());
    VisiblePoints v;
    size_t cap = std::min(n, std::max<size_t>(capacity_, size_t(1) << 16));
    for (;;) {
      v.index.resize(cap);
      v.rgb.resize(3 * cap);
      v.mask.resize(cap);
      v.xyz_cam.resize(3 * cap);
      v.xyz_world.resize(3 * cap);
      int64_t m = 0;
      dev_.check(pcp_frame_visible(dev_.get(), keyframe, static_cast<int64_t>(cap), v.index.data(), v.rgb.data(), v.mask.data(),
                                   v.xyz_cam.data(), v.xyz_world.data(), &m));
      const size_t sm = static_cast<size_t>(m);
      if (sm > cap) {  // the library wrote the first `cap` records and reported the true count
        cap = std::min(n, sm + sm / 8);
        continue;
      }
      capacity_ = std::max(capacity_, sm + sm / 8);
      v.index.resize(sm);
      v.rgb.resize(3 * sm);
      v.mask.resize(sm);
      v.xyz_cam.resize(3 * sm);
      v.xyz_world.resize(3 * sm);
      return v;
    }
  }

 private:
  Device &dev_;
  mutable size_t capacity_ = 0;  // records of the largest keyframe so far (+ 1/8)
};

// vlcal::VisualLiDARCalibration (PCP/src/calibrate.cpp:42-126): NID-based refinement of
// T_camera_lidar on the z-buffer-culled keyframe clouds
class VisualLiDARCalibration {
 public:
  explicit VisualLiDARCalibration(Device &dev) : dev_(dev) {}
  // returns T_camera_lidar_optimized as a 4x4 row-major matrix (identity initial guess, 16 bins,
  // <= 10 outer iterations: calibrate.cpp:45-51, visual_camera_calibration.hpp:17,28)
  std::vector<double> calibrate(double *final_cost = nullptr) const {
    int64_t pts = 0;
    dev_.check(pcp_nid_prepare(dev_.get(), &pts));
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<double> T(16);
    int32_t evals = 0;
    dev_.check(pcp_nid_optimize(dev_.get(), I, 16, 10, T.data(), final_cost, &evals));
    return T;
  }

 private:
  Device &dev_;
};

struct SmoothedCloud {  // pcl::PointCloud<pcl::PointNormal> mls_points + corresponding_input_indices
  std::vector<float> xyz, normal, curvature;
  std::vector<int32_t> index;
};

// One chunk of CloudSmooth::processAndColorizeStreamed: the rows that received a colour (removePointsWithNoColor done)
struct ColouredChunk {
  std::vector<int32_t> index;  // source index the smoothing chain reports (the uploaded, unsmoothed cloud)
  std::vector<float> xyz;      // 3 per row: the smoothed point
  std::vector<uint8_t> rgb;    // 3 per row
  std::vector<uint8_t> label;  // fused label per row (label fusion on), else empty
};
// Formatted rows handed to a text sink (the device writer): `rows` whole rows in `bytes` bytes; the buffer is reused
struct TextRows {
  const char *text;
  size_t bytes, rows;
  bool labelled;  // coloured rows: XYZRGBMASK text (the fused label as segmentMask) instead of XYZRGB text
};
// rows per window of the text forms: bounds the host buffer (105 B x 2^20 for PointNormal rows) whatever the chunk size
constexpr int64_t kTextWindowRows = int64_t(1) << 20;
struct StreamedColourStats {
  int32_t chunks = 0;
  int64_t rows = 0, coloured = 0;            // smoothed rows, rows with a colour
  double sweep_a_s = 0.0, sweep_b_s = 0.0;  // host-clock seconds, the sinks included
  int64_t voxels = 0;                       // output_leaf > 0: rows of the voxel-grid output
  double voxel_add_s = 0.0, voxel_finish_s = 0.0;
  double ortho_add_s = 0.0;                 // setOrthoAccumulate(true): the chunks' pcp_ortho_add calls
};
// the largest cloud one upload takes (pcp_upload_cloud*: n < 2^31)
constexpr int64_t kMaxUploadPoints = (int64_t(1) << 31) - 1;

class CloudSmooth {
 public:
  explicit CloudSmooth(Device &dev) : dev_(dev) { pcp_default_mls_params(&params_); }
  CloudSmooth(Device &dev, const pcp_mls_params &p) : dev_(dev), params_(p) {}
  void initialize(const pcp_mls_params &p) { params_ = p; }  // CloudSmooth::initialize(MLSParameters)
  // MLSParameters slp_upsampling_radius / slp_upsampling_stepsize (cloudSmooth.hpp:28-29; the reference's 0.05 / 0.01,
  // PointCloudProcessor.cpp:74-75, are the defaults): SAMPLE_LOCAL_PLANE's disk, applied to the context before each run
  void setLocalPlaneSampling(double radius, double step) {
    slp_radius_ = radius;
    slp_step_ = step;
  }
  // processAndColorizeStreamed*: every chunk, once coloured, is also added to the orthographic map the caller has begun on the
  // colour device (Device::orthoBegin), under index_base = the rows of the chunks before it -- its rows' places in the
  // concatenated smoothed cloud; the caller finishes, fetches and ends the map after the call (Device::orthoFetch / orthoEnd)
  void setOrthoAccumulate(bool on) { ortho_accumulate_ = on; }
  // the whole CloudSmooth::process: SOR -> MLS (+ upsampling) -> SOR (cloudSmooth.cpp:109-164)
  SmoothedCloud processWithOutlierRemoval() const { return run(true); }
  // pcl::MovingLeastSquares::process alone
  SmoothedCloud process() const { return run(false); }
  // the rows the last process* call returned are still the device's smoothing result (Device::mlsFetchAscii reads them); false
  // after the streamed fallback, which gathers its chunks on the host
  bool resultResident() const { return resident_; }
  // The whole CloudSmooth::process through the streamed form (pcp_cloud_smooth_stream_begin / _next): any size of upsampled
  // cloud -- the reference's VOXEL_GRID_DILATION 1 mm x 4 (PointCloudProcessor.cpp:78-81) makes ~2.8e9 rows of a 10 M-point
  // map, more than one result holds.  sink(const SmoothedCloud &chunk) receives the survivors of the trailing outlier
  // removal chunk by chunk, in the order the one-shot form returns them; total_rows (nullable): rows before that filter.
  // Returns the rows kept.
  // hold_device_memory: leave the stream's distances on the device (4 B per row: 11 GB for a 10 M-point map) for the next call
  // instead of freeing them (pcp_cloud_smooth_stream_end).
  // max_rows: a caller that gathers the chunks into ONE cloud for a later upload passes kMaxUploadPoints: more kept rows
  // than that end the call before the first chunk is fetched (the colour stage could not take them; processAndColorizeStreamed
  // -- `--streamColour 1` on the command line -- colours such a cloud chunk by chunk).
  template <class Sink>
  int64_t processWithOutlierRemovalStreamed(int64_t chunk_capacity, Sink &&sink, int64_t *total_rows = nullptr,
                                            bool hold_device_memory = false, int64_t max_rows = -1) const {
    int64_t total = 0, kept = 0;
    int32_t chunks = 0;
    dev_.check(pcp_cloud_smooth_stream_begin(dev_.get(), &params_, chunk_capacity, &total, &kept, &chunks));
    if (total_rows) *total_rows = total;
    if (max_rows >= 0 && kept > max_rows) {
      dev_.check(pcp_cloud_smooth_stream_end(dev_.get()));
      throw std::runtime_error("pcp_hip: the smoothed cloud has " + std::to_string(kept) + " rows, more than one upload takes (" +
                               std::to_string(max_rows) + "): it cannot be gathered for the colour stage; colour it chunk by chunk "
                               "(CloudSmooth::processAndColorizeStreamed, --streamColour 1 on the command line)");
    }
    SmoothedCloud s;
    for (;;) {
      int64_t m = 0;
      dev_.check(pcp_cloud_smooth_stream_next(dev_.get(), &m));
      if (m == 0) break;
      fetch(m, s);
      sink(static_cast<const SmoothedCloud &>(s));
    }
    if (!hold_device_memory) dev_.check(pcp_cloud_smooth_stream_end(dev_.get()));
    return kept;
  }

  // CloudSmooth::process followed by the colourisation of the smoothed cloud (PointCloudProcessor.cpp:139-145, 474-602) for
  // clouds whose smoothed rows exceed one upload -- nothing of the smoothed cloud is gathered on the host.  A chunk of the
  // chain's voxel order is an index shard in time: the depth maps are a MIN over all points and a point's colour depends only
  // on its own projection, the merged maps and the images, so the chunks' results concatenate to the one-shot result bit for
  // bit (DESIGN.md "Streamed colourisation").  This object's device holds the cloud to smooth; `colour` is a second context
  // on the same GPU with camera, keyframes and images (masks and pcp_set_label_fusion for labels) set.  Every chunk reaches
  // it device to device (pcp_upload_cloud_from_result).
  //   sweep A  per chunk: depth pass over all keyframes, merged into colour's accumulator; smoothed(chunk, kept_rows) receives
  //            the chunk's rows -- the <stem>_mls.pcd rows as they come; kept_rows, their total, is known from the start;
  //   sweep B  the stream rewound: depth pass (tile masks), the accumulator applied, colours, compaction on the device;
  //            sink(const ColouredChunk &) receives every chunk's coloured rows.
  // output_leaf > 0: the coloured rows are also reduced on `colour` to one row per occupied voxel of that edge (pcp_voxel_reduce_*):
  // begin before sweep B, one add per coloured chunk, finish after the sweep; the caller then reads colour.voxelReduceFetch()
  // and ends it (colour.voxelReduceEnd()).  fetch_rows = false: the chunks are compacted with capacity 0 -- only the count
  // comes back, the sink is not called -- so with output_leaf nothing but the reduced rows leaves the device.
  template <class Sink, class SmoothedSink>
  StreamedColourStats processAndColorizeStreamed(Device &colour, int64_t chunk_capacity, Sink &&sink, SmoothedSink &&smoothed,
                                                 bool fuse_labels = false, float output_leaf = 0.0f, bool fetch_rows = true) const {
    pcp_context *src = dev_.get(), *dst = colour.get();
    SmoothedCloud s;
    ColouredChunk out;
    std::vector<int32_t> source;
    return streamedSweeps(
        colour, chunk_capacity,
        [&](int64_t m, int64_t kept) {
          fetch(m, s);
          smoothed(static_cast<const SmoothedCloud &>(s), kept);
        },
        [&](int64_t m) {
          int64_t coloured = 0;
          if (!fetch_rows) {
            colour.check(pcp_colour_compact(dst, 0, nullptr, nullptr, nullptr, nullptr, &coloured));
            return coloured;
          }
          const size_t sm = static_cast<size_t>(m);
          out.index.resize(sm);
          out.xyz.resize(3 * sm);
          out.rgb.resize(3 * sm);
          out.label.resize(fuse_labels ? sm : 0);
          colour.check(pcp_colour_compact(dst, m, out.index.data(), out.xyz.data(), out.rgb.data(), fuse_labels ? out.label.data() : nullptr,
                                          &coloured));
          const size_t sc = static_cast<size_t>(coloured);
          out.index.resize(sc);
          out.xyz.resize(3 * sc);
          out.rgb.resize(3 * sc);
          out.label.resize(fuse_labels ? sc : 0);
          if (coloured == 0) return coloured;
          source.resize(sm);
          dev_.check(pcp_mls_fetch(src, m, nullptr, nullptr, nullptr, source.data()));
          for (size_t k = 0; k < sc; ++k) out.index[k] = source[static_cast<size_t>(out.index[k])];
          sink(static_cast<const ColouredChunk &>(out));
          return coloured;
        },
        output_leaf);
  }
  // The same two sweeps with the rows delivered as TEXT, formatted on the device (the device PCD writer): smoothed(const
  // TextRows &, kept_rows) receives each chunk's PointNormal rows in sweep A, sink(const TextRows &) each chunk's coloured rows in
  // sweep B -- as XYZRGB text and, with fuse_labels, once more as XYZRGBMASK text (labelled) -- in windows of at most
  // window_rows rows through one reused buffer, so a 2^28-voxel chunk never needs its 12 GB of text at once.  The windows in
  // order are the bytes the host writers print of the binary sinks' rows.
  template <class Sink, class SmoothedSink>
  StreamedColourStats processAndColorizeStreamedText(Device &colour, int64_t chunk_capacity, Sink &&sink, SmoothedSink &&smoothed,
                                                     bool fuse_labels = false, int64_t window_rows = kTextWindowRows,
                                                     float output_leaf = 0.0f, bool fetch_rows = true) const {
    std::vector<char> text;
    return streamedSweeps(
        colour, chunk_capacity,
        [&](int64_t m, int64_t kept) {
          for (int64_t first = 0; first < m;) {
            const Device::TextWindow w = dev_.mlsFetchAscii(first, window_rows, text);
            if (w.rows == 0) break;
            smoothed(TextRows{text.data(), static_cast<size_t>(w.bytes), static_cast<size_t>(w.rows), false}, kept);
            first += w.rows;
          }
        },
        [&](int64_t) {
          int64_t coloured = 0;
          if (!fetch_rows) {
            colour.check(pcp_colour_compact(colour.get(), 0, nullptr, nullptr, nullptr, nullptr, &coloured));
            return coloured;
          }
          for (int labelled = 0; labelled <= (fuse_labels ? 1 : 0); ++labelled)
            for (int64_t first = 0;;) {
              const Device::TextWindow w = colour.colourCompactAscii(labelled != 0, first, window_rows, text);
              if (w.rows == 0) break;
              sink(TextRows{text.data(), static_cast<size_t>(w.bytes), static_cast<size_t>(w.rows), labelled != 0});
              first += w.rows;
              if (!labelled) coloured += w.rows;
            }
          return coloured;
        },
        output_leaf);
  }
  template <class Sink>
  StreamedColourStats processAndColorizeStreamed(Device &colour, int64_t chunk_capacity, Sink &&sink) const {
    return processAndColorizeStreamed(colour, chunk_capacity, sink, [](const SmoothedCloud &, int64_t) {});
  }

 private:
  // the two sweeps of processAndColorizeStreamed: after_a(rows, kept_rows) once per chunk of sweep A (the chunk is this
  // device's smoothing result), after_b(rows) -> coloured rows once per chunk of sweep B (the chunk is coloured on `colour`)
  template <class AfterA, class AfterB>
  StreamedColourStats streamedSweeps(Device &colour, int64_t chunk_capacity, AfterA &&after_a, AfterB &&after_b,
                                     float output_leaf = 0.0f) const {
    using clock = std::chrono::steady_clock;
    pcp_context *src = dev_.get(), *dst = colour.get();
    StreamedColourStats st;
    int64_t total = 0, kept = 0;
    int32_t frames = pcp_frame_count(dst);
    dev_.check(pcp_set_mls_local_plane(src, slp_radius_, slp_step_));
    colour.check(pcp_depth_accum_reset(dst));
    dev_.check(pcp_cloud_smooth_stream_begin(src, &params_, chunk_capacity, &total, &kept, &st.chunks));
    struct EndStream {  // also on the way out of an exception
      pcp_context *c;
      ~EndStream() { (void)pcp_cloud_smooth_stream_end(c); }
    } end_stream{src};
    auto t0 = clock::now();
    for (int32_t c = 0; c < st.chunks; ++c) {  // (chunks without rows are skipped by _next: the calls left over return 0)
      int64_t m = 0, n = 0;
      dev_.check(pcp_cloud_smooth_stream_next(src, &m));
      if (m == 0) continue;
      st.rows += m;
      colour.check(pcp_upload_cloud_from_result(dst, src, &n));
      colour.check(pcp_depth_pass(dst, 0, frames));
      colour.check(pcp_depth_accum_merge(dst));
      after_a(m, kept);
    }
    colour.check(pcp_synchronize(dst));
    st.sweep_a_s = std::chrono::duration<double>(clock::now() - t0).count();
    t0 = clock::now();
    if (output_leaf > 0.0f) colour.voxelReduceBegin(output_leaf);
    dev_.check(pcp_cloud_smooth_stream_seek(src, 0));
    int64_t rows_before = 0;
    for (int32_t c = 0; c < st.chunks; ++c) {
      int64_t m = 0, n = 0;
      dev_.check(pcp_cloud_smooth_stream_next(src, &m));
      if (m == 0) continue;
      colour.check(pcp_upload_cloud_from_result(dst, src, &n));
      colour.check(pcp_depth_pass(dst, 0, frames));  // builds this chunk's tile masks, as on a shard before the all-reduce(MIN)
      colour.check(pcp_depth_accum_apply(dst));
      colour.check(pcp_colorize_from_depth(dst, nullptr, nullptr));
      if (output_leaf > 0.0f) {
        colour.check(pcp_synchronize(dst));  // (the colour pass is asynchronous: the clock below takes the add alone)
        const auto t1 = clock::now();
        (void)colour.voxelReduceAdd();
        st.voxel_add_s += std::chrono::duration<double>(clock::now() - t1).count();
      }
      if (ortho_accumulate_) {
        colour.check(pcp_synchronize(dst));
        const auto t1 = clock::now();
        (void)colour.orthoAdd(rows_before);
        st.ortho_add_s += std::chrono::duration<double>(clock::now() - t1).count();
      }
      rows_before += m;
      st.coloured += after_b(m);
    }
    if (output_leaf > 0.0f) {
      const auto t1 = clock::now();
      st.voxels = colour.voxelReduceFinish();
      st.voxel_finish_s = std::chrono::duration<double>(clock::now() - t1).count();
    }
    st.sweep_b_s = std::chrono::duration<double>(clock::now() - t0).count();
    return st;
  }
  void fetch(int64_t m, SmoothedCloud &s) const {
    const size_t sm = static_cast<size_t>(m);
    s.xyz.resize(3 * sm);
    s.normal.resize(3 * sm);
    s.curvature.resize(sm);
    s.index.resize(sm);
    dev_.check(pcp_mls_fetch(dev_.get(), m, s.xyz.data(), s.normal.data(), s.curvature.data(), s.index.data()));
  }
  SmoothedCloud run(bool with_sor) const {
    resident_ = false;
    dev_.check(pcp_set_mls_local_plane(dev_.get(), slp_radius_, slp_step_));
    int64_t m = 0;
    int rc = with_sor ? pcp_cloud_smooth(dev_.get(), &params_, &m) : pcp_mls_process(dev_.get(), &params_, &m);
    if (with_sor && rc == PCP_ERR_NOMEM && params_.upsampling == PCP_UPSAMPLING_VOXEL_GRID_DILATION) {
      // more upsampled points than one result holds: the streamed chain, gathered on the host (the caller asked for one cloud)
      SmoothedCloud all;
      // (as long as the colour stage can take the one cloud: beyond an upload's size the call ends here, before 90 GB are gathered)
      processWithOutlierRemovalStreamed(int64_t(1) << 28, [&](const SmoothedCloud &c) {
        all.xyz.insert(all.xyz.end(), c.xyz.begin(), c.xyz.end());
        all.normal.insert(all.normal.end(), c.normal.begin(), c.normal.end());
        all.curvature.insert(all.curvature.end(), c.curvature.begin(), c.curvature.end());
        all.index.insert(all.index.end(), c.index.begin(), c.index.end());
      }, nullptr, false, kMaxUploadPoints);
      return all;
    }
    dev_.check(rc);
    SmoothedCloud s;
    const size_t sm = static_cast<size_t>(m);
    s.xyz.resize(3 * sm);
    s.normal.resize(3 * sm);
    s.curvature.resize(sm);
    s.index.resize(sm);
    dev_.check(pcp_mls_fetch(dev_.get(), m, s.xyz.data(), s.normal.data(), s.curvature.data(), s.index.data()));
    resident_ = true;
    return s;
  }

  Device &dev_;
  mutable bool resident_ = false;
  pcp_mls_params params_;
  double slp_radius_ = 0.05, slp_step_ = 0.01;
  bool ortho_accumulate_ = false;
};

}  // namespace pcp_amd
