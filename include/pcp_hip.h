/*
 * pcp_hip.h -- C ABI of libpcp_hip.so: the MI355X (gfx950) implementation of
 * PointCloudProcessor's colourisation / view-culling / MLS hot path.
 *
 * The reference (ChunLI-666/PointCloudProcessor @2024_10_08) has no FFI or
 * plugin interface: the path is reached through C++ member calls.  Every entry
 * point below names the reference call site it replaces (PCP/ =
 * PointCloudProcessor/ in the reference tree); INTEGRATION.md shows the shim a
 * maintainer adds at each site.
 *
 * Conventions
 *  - plain C types, caller-owned host buffers, no exceptions across the
 *    boundary: every call returns PCP_OK (0) or a negative error class and
 *    pcp_last_error() holds the message (the C++ shim rethrows
 *    std::runtime_error so that main.cpp:64-68 still maps it to exit code -2);
 *  - the library owns all device memory behind the opaque handle; no host
 *    pointer is retained after a call returns;
 *  - one calling thread per handle (the reference makes every hot-path call
 *    from its main thread, PointCloudProcessor.cpp:1007-1032);
 *  - there is no CPU fallback: without a usable HIP device pcp_create() fails.
 *  - results: pixel / cell indices, depth maps and keep masks are bit-exact
 *    with the CPU restatement in oracle/; colours and MLS outputs within 1e-4
 *    relative.
 */
#ifndef PCP_HIP_H
#define PCP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCP_ABI_VERSION 6 /* 2: pcp_cull_params grew cull_mode / match_mode; pcp_set_image_adjust
                             3: PCP_CULL_HPR, pcp_cull_params.hpr_flip_radius, pcp_hpr_stats
                             4: entry points added, no layout changed: pcp_sor_partial / pcp_sor_finish /
                                pcp_sor_chunk_points, pcp_hull_flags_import; PCP_DEPTH_BATCHED accepts PCP_CULL_HPR
                             5: no entry point or layout changed; pcp_cull_frame's out_keep, pcp_sor_partial's out_chunk_sums,
                                pcp_sor_finish's all_chunk_sums / out_keep may be DEVICE memory of the context's GPU (the
                                multi-GPU host exchanges them with RCCL instead of through the host)
                             6: entry points added: pcp_cloud_smooth_stream_begin / _next / _end / _stats (the whole enableMLS chain
                                with its trailing outlier removal over a chunked voxel dilation); pcp_hpr_stats reports
                                candidates = -1 after a call served from the whole-run bits;
                                entry points added, no layout changed: pcp_colour_smooth_local / _packed (PCP_K_COLOUR_SMOOTH = 12,
                                PCP_K_COUNT 13);
                                entry points added, no layout changed: pcp_upload_image_jpeg / _async (pcp_jpeg_header);
                                entry points added, no layout changed: pcp_set_mls_local_plane / pcp_mls_local_plane_samples
                                (pcp_mls_params.upsampling accepts PCP_UPSAMPLING_SAMPLE_LOCAL_PLANE; older libraries refuse
                                it with PCP_ERR_INVALID);
                                entry points added, no layout changed: pcp_set_label_fusion / pcp_colour_labels /
                                pcp_colour_labels_device (fused segmentation labels; off by default);
                                entry points added, no layout changed: pcp_upload_cloud_from_result, pcp_depth_accum_reset / _merge /
                                _apply / _device, pcp_cloud_smooth_stream_seek, pcp_colour_compact (streamed colourisation: a
                                smoothed cloud larger than one upload coloured chunk by chunk; nothing runs unless called);
                                entry points added, no layout changed: pcp_ascii_row_bound, pcp_ascii_rows_host, pcp_ascii_rows,
                                pcp_colour_compact_ascii, pcp_mls_fetch_ascii (the device PCD writer; nothing runs unless called);
                                entry points added, no layout changed: pcp_ascii_parse_host, pcp_ascii_parse, pcp_ascii_parse_limit
                                (the device PCD reader; nothing runs unless called);
                                entry points added, no layout changed: pcp_view_pair_stats / _counters, pcp_exposure_gains,
                                pcp_set_frame_gains (per-keyframe exposure gains; off by default);
                                entry points added, no layout changed: pcp_voxel_reduce_begin / _add / _finish / _fetch / _stats / _end,
                                pcp_voxel_reduce_host (voxel-grid output; nothing runs unless called);
                                entry points added, no layout changed: pcp_estimate_normals, pcp_normals_fetch,
                                pcp_normals_moments_host, pcp_frame_geometry (geometry maps; nothing runs unless called);
                                entry points added, no layout changed: pcp_mask_edt, pcp_mask_edt_frames, pcp_mask_edt_host
                                (mask distance maps; nothing runs unless called);
                                entry points added, no layout changed: pcp_crack_width, pcp_crack_width_host (crack width maps;
                                nothing runs unless called);
                                entry points added, no layout changed: pcp_crack_fuse_begin / _add / _fetch / _end / _host,
                                pcp_crack_components / _fetch / _host (crack widths on the map; nothing runs unless called);
                                entry points added, no layout changed: pcp_crack_lengths / _fetch / _host, pcp_crack_paths_fetch
                                (crack lengths on the map; nothing runs unless called);
                                entry points added, no layout changed: pcp_crack_skeleton / _nodes_fetch / _edges_fetch /
                                _cracks_fetch / _host (crack skeletons on the map; nothing runs unless called);
                                entry points added, no layout changed: pcp_ortho_begin / _add / _add_packed / _finish / _fetch /
                                _stats / _end, pcp_ortho_host, pcp_ortho_fit_frame_host (orthographic maps; nothing runs unless
                                called);
                                entry points added, no layout changed: pcp_default_balance_params, pcp_set_image_balance,
                                pcp_image_balance, pcp_image_balance_host, pcp_gamma_table_host (keyframe colour balance at upload;
                                off by default);
                                entry points added, no layout changed: pcp_ortho_texture, pcp_ortho_texture_points_host
                                (orthophotos; nothing runs unless called);
                                entry points added, no layout changed: pcp_facets / _fetch / _host, pcp_facet_plane_host,
                                pcp_ortho_add_facet (planar facets of the map; nothing runs unless called);
                                entry points added, no layout changed: pcp_ortho_begin_cyl, pcp_ortho_cyl_host, pcp_cyl_angle_host,
                                pcp_cyl_fit_host (cylindrical facets and their unrolled maps; nothing runs unless called);
                                entry points added, no layout changed: pcp_ortho_texture_cyl, pcp_ortho_texture_points_cyl_host,
                                pcp_cyl_sincos_host (orthophotos of unrolled maps; nothing runs unless called);
                                entry points added, no layout changed: pcp_crack_directions / _fetch / _host, pcp_crack_axis_host
                                (crack directions on the map; nothing runs unless called);
                                entry points added, no layout changed: pcp_crack_branches / _fetch / _host,
                                pcp_crack_branch_edges_fetch / _cracks_fetch, pcp_crack_branch_lengths_host (crack branches on the
                                map; nothing runs unless called);
                                entry points added, no layout changed: pcp_ortho_defects / _fetch / _table / _host
                                (surface defects on ortho maps; nothing runs unless called);
                                entry points added, no layout changed: pcp_default_compare_params, pcp_compare_set_base,
                                pcp_compare / _fetch / _host / _end (map comparison with an earlier survey; nothing runs unless
                                called);
                                entry points added, no layout changed: pcp_default_register_params, pcp_compare_register /
                                _register_sums / _register_host, pcp_compare_base_transform, pcp_compare_set_base_transform,
                                pcp_register_solve_host (registration of the earlier survey onto the map; nothing runs unless
                                called);
                                entry points added, no layout changed: pcp_default_coarse_params, pcp_coarse_descriptors / _fetch /
                                _host, pcp_coarse_match / _fetch / _host, pcp_coarse_score / _host, pcp_coarse_hypothesis_host,
                                pcp_coarse_refit_host, pcp_compare_base_normals_fetch, pcp_compare_register_coarse / _host (coarse
                                registration of the earlier survey from any pose; nothing runs unless called) */

#define PCP_OK 0
#define PCP_ERR_INVALID (-1) /* bad argument */
#define PCP_ERR_STATE (-2)   /* call order: camera / cloud / frames / images missing */
#define PCP_ERR_DEVICE (-3)  /* HIP runtime failure */
#define PCP_ERR_NOMEM (-4)   /* host or device allocation failed */
#define PCP_ERR_RANGE (-5)   /* frame index or capacity out of range */

typedef struct pcp_context pcp_context;

/* PCP/include/FrameData.hpp:9-12 (Pose); odometry line "ts x y z qw qx qy qz",
 * PCP/src/PointCloudProcessor.cpp:970-978. */
typedef struct pcp_pose {
  double x, y, z, qw, qx, qy, qz;
} pcp_pose;

/* K_camera / D_camera, PCP/src/PointCloudProcessor.cpp:57-62; image size used by
 * generateColorMap (:754); ViewCulling image_size hard-coded {4096,3000} (:206,:525). */
typedef struct pcp_camera {
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
  int32_t image_width, image_height;
  int32_t cull_width, cull_height;
} pcp_camera;

/* Which of ViewCulling's two routines decides the candidates (pcp_cull_params.cull_mode). */
#define PCP_CULL_ZBUFFER 0 /* ViewCulling::view_culling, view_culling.cpp:52-174 (the routine north_star names; its
                              call is commented out at :43) */
#define PCP_CULL_HPR_CANDIDATES 1 /* ONLY the candidate filter of ViewCulling::hidden_points_removal, view_culling.cpp:
                              276-288: z > 0 and 0 <= (int)u < cull_width and 0 <= (int)v < cull_height, every candidate
                              kept -- a frustum cull, no occlusion test.  It is a SUPERSET of what the reference binary
                              keeps: at map density the hull below drops most of these candidates (C3 scene, 10 M points:
                              between 3 % and 90 % of a keyframe's candidates, profiles/r03_hpr_retention.json). */
#define PCP_CULL_HPR 2 /* ViewCulling::hidden_points_removal, view_culling.cpp:266-334, the routine the reference binary
                              calls (:46): the candidates above, flipped about a sphere of radius hpr_flip_radius
                              (:291-292), the origin appended (:297); visible = the vertices of the convex hull of that
                              set other than the origin (qhull, :302-329).  Computed on the device, per candidate, with
                              checked certificates (csrc/pcp_hpr.hip); the keep set is the exact set of extreme points,
                              from which qhull's differs by the points within its round-off (~1e-10 m) of a facet.  Kept
                              points are reported in input order (the reference lists them in qhull's vertex order). */

/* How a visible sample is credited to map points (pcp_cull_params.match_mode), PointCloudProcessor.cpp:554-592. */
#define PCP_MATCH_IDENTITY 0 /* the sample of point i is credited to point i, scores from the transform output p_c
                              (SURVEY.md Appendix B3 "identity mode"; ~2 % faster steps) */
#define PCP_MATCH_ROUNDTRIP 1 /* (default) the reference's arithmetic: p_w = c2w p_c in fp32 (:555), the sample is dropped unless
                              |p_w - p_i|^2 < f32(1e-5^2) in fp32 (what radiusSearch(1e-5) tests for point i itself,
                              :571), scores from p_c' = c2w.inverse() p_w in fp32 (:578-579).  Samples that the
                              reference's kd-tree would ALSO credit to other map points closer than 10 um to p_w are
                              not credited to them here (needs map points < ~20 um apart): PCP_MATCH_RADIUS does. */
#define PCP_MATCH_RADIUS 2 /* the reference's whole match-back (:480-482,555,571-592): every map point j with
                              |p_w - p_j|^2 < f32(1e-5^2) (fp32 L2_Simple, strict <) receives the sample, j = i included
                              when it passes; per point, samples arrive in (keyframe, input index) order.  Built on
                              ROUNDTRIP: points with no other map point within R_c = (1e-5 + E)(1 + 1e-3), E a proven
                              bound of the fp32 round-trip displacement (DESIGN.md "Radius match-back"), are served by the
                              colour pass as in ROUNDTRIP; the others (set A) by a fix-up kernel over a neighbour table
                              that the first colour pass in this mode builds.  Costs sum_{j in A} |row(j)| x keyframes.
                              Not available on an index shard (PCP_DEPTH_BATCHED): the colour pass returns
                              PCP_ERR_STATE.  A sample displaced further than E (never, by the proof) makes the colour
                              pass fail rather than return a result.  Libraries before this mode reject it in
                              pcp_set_camera with PCP_ERR_INVALID: that is how a caller detects support. */

/* vlcal::ViewCullingParams, PCP/include/vlcal/calib/view_culling.hpp:10-19, plus
 * the constants 14 (view_culling.cpp:63) and 0.05 (:157). */
typedef struct pcp_cull_params {
  int32_t enable_depth_buffer_culling;
  int32_t downsample_factor;
  double depth_slack;
  int32_t cull_mode;  /* PCP_CULL_ZBUFFER (default) / PCP_CULL_HPR_CANDIDATES / PCP_CULL_HPR */
  int32_t match_mode; /* PCP_MATCH_ROUNDTRIP (default) / PCP_MATCH_IDENTITY / PCP_MATCH_RADIUS */
  double hpr_flip_radius; /* ViewCullingParams::hidden_points_removal_max_z = 90000 (view_culling.hpp:14) */
} pcp_cull_params;

/* pcp_mls_params.upsampling: pcl::MovingLeastSquares::UpsamplingMethod as CloudSmooth::process selects it
 * (PCP/src/cloudSmooth.cpp:133-152).  These are this library's codes, not the positions in the reference's enum
 * (cloudSmooth.hpp:13-19 orders SAMPLE_LOCAL_PLANE 0 .. VOXEL_GRID_DILATION 2); RANDOM_UNIFORM_DENSITY has none (its
 * samples come from an unseeded generator shared by threads: no run of the reference can be reproduced). */
#define PCP_UPSAMPLING_NONE 0
#define PCP_UPSAMPLING_SAMPLE_LOCAL_PLANE 1 /* a disk of samples per fitted point, pcp_set_mls_local_plane */
#define PCP_UPSAMPLING_VOXEL_GRID_DILATION 3
/* most samples per axis of the SAMPLE_LOCAL_PLANE table: radius / step <= PCP_MLS_SLP_MAX_RATIO */
#define PCP_MLS_SLP_MAX_RATIO 512

/* MLSParameters, PCP/include/cloudSmooth.hpp:21-36; values
 * PCP/src/PointCloudProcessor.cpp:67-86. */
typedef struct pcp_mls_params {
  double search_radius;
  double sqr_gauss_param;
  int32_t polynomial_order;
  int32_t compute_normals;
  int32_t upsampling; /* PCP_UPSAMPLING_NONE / _SAMPLE_LOCAL_PLANE / _VOXEL_GRID_DILATION (this library's codes) */
  int32_t vgd_iterations;
  float vgd_voxel_size;
  int32_t sor_mean_k;   /* 60  (PointCloudProcessor.cpp:84) */
  double sor_std_mul;   /* 0.7 (PointCloudProcessor.cpp:86) */
} pcp_mls_params;

/* kernel ids for pcp_timing_get() */
enum {
  PCP_K_PROJECT = 0,    /* single-frame projection (the roofline kernel) */
  PCP_K_DEPTH = 1,      /* batched z-buffer MIN pass */
  PCP_K_COLOUR = 2,     /* batched visibility + colour + score + top-5 pass */
  PCP_K_VISIBILITY = 3, /* single-frame keep mask */
  PCP_K_MLS_GRID = 4,   /* MLS cell binning / counting sort */
  PCP_K_MLS_FIT = 5,    /* MLS radius search + polynomial fit + projection */
  PCP_K_MISC = 6,       /* fills, compaction, permutation */
  PCP_K_SOR = 7,        /* StatisticalOutlierRemoval kNN mean distance */
  PCP_K_MLS_VOXEL = 8,  /* upsampling emission (VOXEL_GRID_DILATION, SAMPLE_LOCAL_PLANE) */
  PCP_K_TILE_MASK = 9,  /* tile x keyframe visibility masks (conservative culling) */
  PCP_K_NID = 10,       /* NID joint histograms (value + SE(3) tangent gradient) */
  PCP_K_HPR = 11,       /* hidden_points_removal: flip, binning, per-candidate hull membership */
  PCP_K_COLOUR_SMOOTH = 12, /* smoothColorsWithLocalRegion: records, work items, radius-weighted colour means */
  PCP_K_COUNT = 13
};

/* ---- lifecycle ---------------------------------------------------------- */
int pcp_abi_version(void);
/* device: HIP device ordinal.  Fails (PCP_ERR_DEVICE) when no GPU is usable. */
int pcp_create(int32_t device, pcp_context **out);
void pcp_destroy(pcp_context *ctx);
/* message of the last failing call on ctx (or of pcp_create when ctx == NULL) */
const char *pcp_last_error(const pcp_context *ctx);
/* run on an externally owned hipStream_t (e.g. torch's current stream); NULL = own stream */
int pcp_set_stream(pcp_context *ctx, void *hip_stream);
int pcp_synchronize(pcp_context *ctx);

/* ---- configuration ------------------------------------------------------ */
void pcp_default_camera(pcp_camera *cam);
void pcp_default_cull_params(pcp_cull_params *p);
void pcp_default_mls_params(pcp_mls_params *p);
/* replaces create_camera + ViewCulling ctor, PointCloudProcessor.cpp:522-525 */
int pcp_set_camera(pcp_context *ctx, const pcp_camera *cam, const pcp_cull_params *cull);

/* ---- cloud -------------------------------------------------------------- */
/* SoA fp32 upload of the map (`cloud`, PointCloudProcessor.cpp:148). */
int pcp_upload_cloud(pcp_context *ctx, const float *x, const float *y, const float *z, int64_t n);
/* AoS upload straight from pcl::PointCloud<PointXYZI>::points.data(): x,y,z are
 * the first three floats of every `stride_bytes` record (32 for PointXYZI). */
int pcp_upload_cloud_aos(pcp_context *ctx, const void *points, int64_t n, int64_t stride_bytes);
/* The rows of src's latest smoothing result -- what pcp_mls_fetch returns as out_xyz, from pcp_mls_process*, pcp_cloud_smooth,
 * pcp_mls_stream_next or pcp_cloud_smooth_stream_next -- become the cloud of dst, device to device: exactly the cloud
 * pcp_upload_cloud_aos(dst, fetched_xyz, n, 12) builds (same spatial order, tile spheres and resets).  *out_n (nullable) = its
 * points.  Both contexts on one GPU, else PCP_ERR_INVALID.  dst's stream waits for src's through an event: the caller does not
 * synchronise src.  With dst != src nothing of src changes (an open stream stays open) and src may produce its next result as
 * soon as the call returns.  dst == src is allowed: the rows are copied aside, then the upload proceeds as any upload does (the
 * result and an open stream end).  No smoothing result since src's latest upload: PCP_ERR_STATE.  A result of 0 rows: an empty
 * cloud, PCP_OK. */
int pcp_upload_cloud_from_result(pcp_context *dst, pcp_context *src, int64_t *out_n);
int64_t pcp_cloud_size(const pcp_context *ctx);

/* ---- frames ------------------------------------------------------------- */
/* Host helper: pose -> (w2c, c2w) 3x4 row-major fp32, PointCloudProcessor.cpp:495-519.
 * T_opt: NULL, or a 4x4 row-major fp64 T_camera_lidar_optimized (:504-519). */
int pcp_pose_to_matrices(const pcp_pose *pose, const double *T_opt, float w2c[12], float c2w[12]);
/* Keyframe poses of the run (selectKeyframes output).  T_opt: NULL, 16 doubles
 * (stride 0, NID result) or n_frames*16 (stride 16, per-keyframe manual guess). */
int pcp_set_frames(pcp_context *ctx, const pcp_pose *poses, int32_t n_frames, const double *T_opt,
                   int32_t T_opt_stride);
int32_t pcp_frame_count(const pcp_context *ctx);
/* Decoded BGR8 image of one keyframe (what generateColorMap holds after the HSV
 * round trip, PointCloudProcessor.cpp:716-741), image_height rows of image_width
 * pixels, row_stride_bytes apart (cv::Mat::step). */
int pcp_upload_image(pcp_context *ctx, int32_t frame, const uint8_t *bgr, int64_t row_stride_bytes);
/* The same without waiting for the copy: returns once the transfer is queued on the context's stream.  The
 * host buffer must stay valid and unchanged until pcp_synchronize (or any synchronising call) returns; from
 * pinned memory a sequence of keyframes streams at the PCIe rate with the packing kernels in between. */
int pcp_upload_image_async(pcp_context *ctx, int32_t frame, const uint8_t *bgr, int64_t row_stride_bytes);
/* `count` keyframes first_frame ... that sit one after the other in PINNED host memory, frame_stride_bytes apart (a pinned
 * arena the decoder fills, cv::Mat headers over it): the copy engine moves them in blocks of <= 128 MB (one DMA per block:
 * the PCIe rate, which neither one copy per keyframe nor kernels reading pinned memory in place reach), each block's
 * keyframes are packed from the device copy, consecutive blocks alternate between two streams.  Asynchronous like
 * pcp_upload_image_async.  Pageable or device memory is accepted and handled keyframe by keyframe. */
int pcp_upload_images_block(pcp_context *ctx, int32_t first_frame, int32_t count, const uint8_t *bgr, int64_t row_stride_bytes,
                            int64_t frame_stride_bytes);
/* Both upload calls also take a DEVICE pointer for `bgr` (e.g. frames broadcast or all-gathered over xGMI by a
 * multi-GPU host): the transfer is then ordered after everything already queued on the context's stream
 * (pcp_set_stream), so a collective that produced the bytes on that stream needs no host synchronisation.  Pinned
 * (device-mapped) host memory is read in place by the pack kernel; pageable memory goes through a staging copy. */
/* The image adjustment generateColorMap applies to every keyframe before sampling it
 * (PointCloudProcessor.cpp:722-741): cv::cvtColor(BGR2HSV) on 8-bit pixels, S and V multiplied by
 * saturation_scale / brightness_scale (both 1.0 in the reference, :728-729) with saturate_cast<uchar>, and
 * cv::cvtColor(HSV2BGR).  8-bit HSV is lossy, so this is not the identity even at scale 1.0.
 * enable != 0: images handed to pcp_upload_image / _async afterwards are RAW decoded pixels (cv::imread output)
 * and the library applies the round trip while packing them (fused into the pack kernel, no extra pass).
 * enable == 0 (default): the caller passes what generateColorMap holds AFTER its own cvtColor calls.
 * Arithmetic: the forward half is OpenCV 4.2's integer routine (RGB2HSV_b, hdiv / sdiv tables, h range 180),
 * restated exactly; the backward half is OpenCV 4.2's scalar float routine (HSV2RGB_native, no FMA), whose
 * SIMD / FMA builds may differ from it by one level on some pixels [upstream, parity unpinned: DESIGN.md]. */
int pcp_set_image_adjust(pcp_context *ctx, int32_t enable, float saturation_scale, float brightness_scale);
/* diagnostic: the pixels of one keyframe as the kernels sample them (after pcp_set_image_adjust's round trip when it
 * was enabled at upload): out_bgr image_height*image_width*3 tightly packed, out_mask image_height*image_width
 * (either nullable) */
int pcp_download_image(pcp_context *ctx, int32_t frame, uint8_t *out_bgr, uint8_t *out_mask);
/* A keyframe JPEG, entropy-decoded on the host (host/image_io.hpp jpeg_coefficients) and reconstructed on the device:
 * dequantisation, libjpeg's islow IDCT, fancy upsampling, the YCbCr->BGR tables -- the pixels of cv::imread (:716) bit for
 * bit -- then pcp_set_image_adjust's round trip and the texel pack, as pcp_upload_image does with decoded pixels.
 * Supported: baseline / extended-sequential Huffman, 8 bit, 1 or 3 components, sampling 4:4:4 / 4:2:2 / 4:2:0.
 *
 * The blob (little-endian, every section 16-B aligned from the blob's start, offsets in bytes):
 *   pcp_jpeg_header                       at 0
 *   quantisation tables  ncomp x 64 uint16, natural order, each component's own table      at quant_off
 *   block masks          n_blocks uint64: bit n set = natural position n is nonzero         at mask_off
 *   value offsets        n_blocks uint32: index of the block's first value                  at offset_off
 *   values               n_values int16: each block's nonzero quantised coefficients in natural order
 *                        (DC after prediction, truncated to int16 as the decoder does)      at value_off
 * Blocks are in decode order: for each MCU row, each MCU, each component, its v rows of h blocks (non-interleaved
 * positions follow from the sampling).  quant_off = 144, mask_off = align16(quant_off + 128 ncomp), offset_off =
 * align16(mask_off + 8 n_blocks), value_off = align16(offset_off + 4 n_blocks); the blob is value_off + 2 n_values bytes.
 * The call checks all of it on the host before anything is queued: magic / version, width x height = the camera's image,
 * ncomp 1 or 3, supported sampling, blocks_* / down_* of every component as the frame size implies, the sections inside
 * `bytes`, and every block's offset delta equal to the popcount of its mask; otherwise PCP_ERR_INVALID. */
#define PCP_JPEG_MAGIC 0x4A504350u /* "PCPJ" */
#define PCP_JPEG_VERSION 1
typedef struct pcp_jpeg_component {
  int32_t h, v;                /* sampling factors (component 0: 1x1, 2x1 or 2x2; components 1, 2: 1x1) */
  int32_t blocks_w, blocks_h;  /* blocks of the component's plane, whole MCUs */
  int32_t down_w, down_h;      /* real samples: ceil(width * h / hmax), ceil(height * v / vmax) */
} pcp_jpeg_component;
typedef struct pcp_jpeg_header {
  uint32_t magic, version;
  int32_t width, height, ncomp, reserved; /* reserved: 0 */
  pcp_jpeg_component comp[3];             /* entries >= ncomp: 0 */
  int64_t n_blocks, n_values;
  int64_t quant_off, mask_off, offset_off, value_off;
} pcp_jpeg_header; /* 144 bytes */
/* Same call order and lifetime rules as pcp_upload_image / pcp_upload_image_async; `blob` is host memory (pageable or
 * pinned), `bytes` its size. */
int pcp_upload_image_jpeg(pcp_context *ctx, int32_t frame, const uint8_t *blob, int64_t bytes);
int pcp_upload_image_jpeg_async(pcp_context *ctx, int32_t frame, const uint8_t *blob, int64_t bytes);
/* gray8 segmentation mask (cv::IMREAD_GRAYSCALE, PointCloudProcessor.cpp:775) */
int pcp_upload_mask(pcp_context *ctx, int32_t frame, const uint8_t *gray, int64_t row_stride_bytes);

/* ---- single keyframe (drop-in for the calls inside the per-keyframe loop) -- */
/* transformPointCloud + project (PointCloudProcessor.cpp:521, view_culling.cpp:86-90,
 * PointCloudProcessor.cpp:748-754).  All outputs nullable, length n, input order:
 *   out_cell  z-buffer cell cy*mw+cx; -1 rejected; -2 = candidate outside the /14 map,
 *             reported only when enable_depth_buffer_culling == 0 (where it is kept)
 *   out_pixel colour pixel v*image_width+u; -1 rejected
 *   out_range f32(||p_c||), valid where out_cell != -1 (FLT_MAX elsewhere)
 *   out_xyz_cam 3*n floats, SoA (x[n] y[n] z[n]) camera coordinates
 * With every output NULL the kernel still runs and leaves cell/range on the
 * device (used by bench.py to time the kernel without PCIe traffic). */
int pcp_project_frame(pcp_context *ctx, int32_t frame, int32_t *out_cell, int32_t *out_pixel, float *out_range,
                      float *out_xyz_cam);
/* ViewCulling::cull with the z-buffer routine (view_culling.cpp:23-50,52-174).
 * out_keep n bytes (nullable), out_depth_map (H/14)*(W/14) floats (nullable). */
int pcp_cull_frame(pcp_context *ctx, int32_t frame, uint8_t *out_keep, int64_t *out_kept, float *out_depth_map);
/* cull + generateColorMap + generateSegmentMap + transform to world
 * (PointCloudProcessor.cpp:527-551): the kept and coloured points of one keyframe
 * in input order.  rgb after the mask==255 -> (255,0,0) override when a mask was
 * uploaded.  All outputs nullable; capacity in points; *out_count = true count. */
int pcp_frame_visible(pcp_context *ctx, int32_t frame, int64_t capacity, int32_t *out_index, uint8_t *out_rgb,
                      uint16_t *out_mask, float *out_xyz_cam, float *out_xyz_world, int64_t *out_count);

/* diagnostic: the last hidden_points_removal run on ctx (PCP_CULL_HPR; the latest keyframe of a batched call):
 * out[0] visible, [1] hidden (both counted from the final verdicts), [2] candidates that went to the exact path (neither
 * floating-point certificate held), [3] trial normals, [4] batches of 64 point tests -- of the polygon and exact searches
 * only --, [5] reserved (0), [6] UNRESOLVED (no exact
 * certificate either: exactly degenerate input such as four coplanar flipped points; classified hidden), [7] exact
 * predicate evaluations, [8] grid cells, [9] candidates.
 * After a single-keyframe call (pcp_cull_frame, pcp_frame_visible, NID) that was SERVED FROM THE WHOLE-RUN BITS -- a
 * pcp_depth_pass of this context had taken the keyframe's hull already, or pcp_hull_flags_import had brought it -- nothing
 * was recomputed and there are no tallies of that keyframe: out[0..8] = 0 and out[9] = -1. */
int pcp_hpr_stats(pcp_context *ctx, int64_t out[10]);

/* ---- whole run (pcdColorizationAndSmooth, PointCloudProcessor.cpp:474-602) -- */
/* z-buffer MIN pass for keyframes [frame_begin, frame_end) over the local points */
int pcp_depth_pass(pcp_context *ctx, int32_t frame_begin, int32_t frame_end);
/* device address of the n_frames*(H/14)*(W/14) fp32 depth maps, for the
 * all-reduce(MIN) across point shards (multi-GPU), and its length in floats */
int pcp_depth_maps_device(pcp_context *ctx, void **device_ptr, int64_t *n_floats);
int pcp_download_depth_map(pcp_context *ctx, int32_t frame, float *out_depth_map);
/* Depth-map accumulator: n_frames*(H/14)*(W/14) floats per context that SURVIVE pcp_upload_cloud* / pcp_upload_cloud_from_result
 * (pcp_set_camera, pcp_set_frames and pcp_destroy drop them).  The maps are a MIN over all points, so a cloud handed over in
 * parts -- the chunks of a streamed smoothing chain -- is an index shard in time: merge every part's maps, apply the merged maps
 * to each part again, and the parts' colour results concatenate to the result of the whole cloud, bit for bit.
 *   _reset  allocates the buffer and sets every cell to the maps' "far" value (FLT_MAX);
 *   _merge  accumulator = min(accumulator, the context's maps), all keyframes; every keyframe must have been covered by
 *           pcp_depth_pass since the latest upload, else PCP_ERR_STATE;
 *   _apply  overwrites the context's maps with the accumulator; same precondition (the context's own pcp_depth_pass has built
 *           its tile masks, as on a shard after the all-reduce(MIN));
 *   _device the buffer's device address and length in floats (for an all-reduce(MIN) across GPUs).
 * All four return PCP_ERR_STATE under PCP_CULL_HPR (see pcp_depth_maps_device), the last three before _reset. */
int pcp_depth_accum_reset(pcp_context *ctx);
int pcp_depth_accum_merge(pcp_context *ctx);
int pcp_depth_accum_apply(pcp_context *ctx);
int pcp_depth_accum_device(pcp_context *ctx, void **device_ptr, int64_t *n_floats);
/* Where the single-keyframe calls (pcp_cull_frame, pcp_frame_visible, pcp_nid_prepare) take a keyframe's depth map
 * from.  PCP_DEPTH_OWN (default): each call builds it from the uploaded points, as ViewCulling::view_culling does.
 * PCP_DEPTH_BATCHED: they use the maps pcp_depth_pass left behind -- for a context that holds one index shard of the
 * map, after the caller's all-reduce(MIN) across shards, these ARE the maps of the whole cloud, so the per-keyframe
 * outputs of the shards concatenate to the single-GPU result.  The keyframe must have been covered by pcp_depth_pass. */
#define PCP_DEPTH_OWN 0
#define PCP_DEPTH_BATCHED 1
int pcp_set_depth_source(pcp_context *ctx, int32_t source);
/* PCP_CULL_HPR over index shards: a keyframe's hull is taken over EVERY candidate of the map (view_culling.cpp:291-329), so
 * a context that holds one shard (PCP_DEPTH_BATCHED) cannot decide its points.  The verdicts come from a context that holds
 * the whole map (pcp_cull_frame there returns them, input order) and are handed to the shard here: keep[i] != 0 = point i
 * of THIS context is a hull vertex of `frame` (n flags, host or device memory).  pcp_colour_pass and the single-keyframe
 * calls of the shard then read them where the z-buffer routine reads the merged depth maps. */
int pcp_hull_flags_import(pcp_context *ctx, int32_t frame, const uint8_t *keep);
int pcp_colour_reset(pcp_context *ctx);
/* visibility + colour lookup + scores + per-point top-5 for [frame_begin, frame_end) */
int pcp_colour_pass(pcp_context *ctx, int32_t frame_begin, int32_t frame_end);
/* smoothColors + removePointsWithNoColor flag (PointCloudProcessor.cpp:604-631,
 * hpp:238-252).  out_rgb n*3 (r,g,b), out_has n; optional: out_count n (#views),
 * out_top_score/out_top_rgb(0x00RRGGBB)/out_top_frame n*5 (desc, -1 padded). */
int pcp_colour_finalise(pcp_context *ctx, uint8_t *out_rgb, uint8_t *out_has, int32_t *out_count,
                        float *out_top_score, uint32_t *out_top_rgb, int32_t *out_top_frame);
/* reset + depth_pass(all) + colour_pass(all) + finalise */
int pcp_colorize(pcp_context *ctx, uint8_t *out_rgb, uint8_t *out_has);
/* visibility + colour + top-5 + smoothColors in one launch over ALL keyframes,
 * given depth maps that already cover them (after pcp_depth_pass and, across
 * point shards, the all-reduce(MIN)).  out_* nullable. */
int pcp_colorize_from_depth(pcp_context *ctx, uint8_t *out_rgb, uint8_t *out_has);
/* packed result r | g<<8 | b<<16 | has<<24, n words, one plain device-to-host copy */
int pcp_download_result_packed(pcp_context *ctx, uint32_t *out_rgba);
/* the same copy on the library's copy stream: returns at once, the result buffer is
 * double-buffered so the next run's kernels overlap this transfer; out_rgba (pinned
 * memory for a real overlap) is valid after pcp_synchronize(). */
int pcp_download_result_packed_async(pcp_context *ctx, uint32_t *out_rgba);
/* Blocks the host until the asynchronous download issued BEFORE the latest one has landed (no-op when there is
 * none): the consumer of a two-buffer ring calls it before reusing the older buffer.  It does not wait for any
 * kernel, so the device stays busy, and it keeps the host at most one run ahead of the device -- an unbounded
 * lead (hundreds of queued commands) was measured to slow the steps by 13 %. */
int pcp_download_wait_previous(pcp_context *ctx);
/* device address of the packed per-point result (r | g<<8 | b<<16 | has<<24),
 * valid after pcp_colour_finalise / pcp_colorize, for device-side gathers */
int pcp_colour_result_device(pcp_context *ctx, void **device_ptr, int64_t *n_words);
/* removePointsWithNoColor (PointCloudProcessor.hpp:238-252) on the device: the rows of the current colour result (after
 * pcp_colour_smooth_local: the smoothed one) whose has bit is set, in input order.  out_index m rows of the uploaded cloud,
 * out_xyz 3*m (the uploaded coordinates bit for bit), out_rgb 3*m (r, g, b), out_label m (the fused label); host memory, all
 * nullable, at most `capacity` rows each.  *out_count = the true count m even when capacity is smaller.  No colour result, or
 * out_label asked of a result made without label fusion: PCP_ERR_STATE. */
int pcp_colour_compact(pcp_context *ctx, int64_t capacity, int32_t *out_index, float *out_xyz, uint8_t *out_rgb, uint8_t *out_label,
                       int64_t *out_count);

/* Fused segmentation labels ("Fused segmentation labels"): one label per map point from the masks of the
 * point's top-5 views, where the reference writes every point once per keyframe that sees it
 * (PointCloudProcessor.cpp:533-551, 932-947).  Off by default; with it off every output and every launched kernel is what
 * it was.  With it on, the colour kernels keep each listed view's mask byte m_k (the texel's top byte) and every colour
 * result (pcp_colorize, pcp_colorize_from_depth, pcp_colour_finalise) carries a second word per point, for the same list
 * (s_k, texel_k, f_k), k < M = min(count, 5), that the colour reads:
 *   views = M,  hits = #{k : m_k == 255},  label = floor(sum m_k S_k / sum S_k),  S_k = s_k * 2^26
 * in exact integer arithmetic (S_k is an integer for every fp32 score in [2^-3, 2); final_score gives [0.2, 1]); an
 * unseen point has the word 0.  A single view returns its m, views that are all 255 return 255, and the order of equal
 * scores does not matter.  A score outside [2^-3, 2) makes the result call return PCP_ERR_RANGE (no labels then).
 * The result call reads that flag back: with fusion on it waits for its kernels.
 * Colours and has are bit for bit those of a fusion-off run; pcp_colour_finalise's out_top_rgb stays 0x00RRGGBB.
 * A colour pass over a keyframe without an uploaded mask (pcp_upload_mask) fails with PCP_ERR_STATE before anything is
 * launched.  Changing the switch while a top-5 accumulation is live (after pcp_colour_pass, before pcp_colour_reset)
 * returns PCP_ERR_STATE.  PCP_MATCH_RADIUS is supported: a credited neighbour sample brings its own pixel's mask.  On an
 * index shard (PCP_DEPTH_BATCHED) the labels are rank-local; the shards' arrays concatenate to the one-GPU result.
 * pcp_colour_smooth_local leaves the labels alone. */
int pcp_set_label_fusion(pcp_context *ctx, int32_t enable);
/* label / hits / views of the latest colour result, n bytes each, all nullable, input order; synchronous.  PCP_ERR_STATE
 * unless that result was produced with fusion on. */
int pcp_colour_labels(pcp_context *ctx, uint8_t *out_label, uint8_t *out_hits, uint8_t *out_views);
/* device address of the packed words label | hits<<8 | views<<16 (n words, input order).  One buffer, NOT double-buffered:
 * valid until the next colour result begins (a later pcp_colorize / pcp_colorize_from_depth / pcp_colour_finalise
 * overwrites or invalidates it), so consume it on the context's stream before that call. */
int pcp_colour_labels_device(pcp_context *ctx, void **device_ptr, int64_t *n_words);

/* Exposure gains ("Exposure gains", EG1-EG5): one brightness gain per keyframe from the map points that two
 * keyframes both colour, so that a point's colour no longer jumps where its top-5 list changes by one view (the reference
 * has one hand-set global brightness, PointCloudProcessor.cpp:726-729, and notes the pairwise idea at RGBCloud.hpp:20-25).
 * Off by default; with it unused every output and every launched kernel is what it was.
 *
 * pcp_view_pair_stats: over every point's list (s_k, c_k, f_k), k < M = min(count, 5), and every ordered pair of distinct
 * slots a != b with f_a != f_b whose views are both usable -- luma Y = (77 R + 150 G + 29 B + 128) >> 8 of the view's colour
 * word within [8, 247] --:  n[f_a][f_b] += 1,  sum[f_a][f_b] += Y_a.  Exact integers, independent of the order of
 * accumulation; n is symmetric.  out_n, out_sum: F x F uint64 each, row-major, HOST memory, either nullable.  Valid while a
 * top-5 accumulation is live (after pcp_colour_pass, before pcp_colour_reset / a one-shot call / an upload), else
 * PCP_ERR_STATE; more than 4096 keyframes: PCP_ERR_RANGE.  On an index shard (PCP_DEPTH_BATCHED) the matrices are the
 * shard's own points': they are ADDITIVE over shards (and over the chunks of a streamed cloud); the caller sums them.
 * PCP_EXPOSURE_TABLE_LOG2=k (0..10) shrinks the kernel's per-workgroup table to 2^k slots (tests of its overflow path).
 * pcp_view_pair_stats_counters: of the latest call -- out[0] 64-bit adds to global memory issued when the workgroups'
 * tables were flushed, [1] adds issued directly because a table was full, [2] wavefront-level partial sums, [3]
 * workgroups, [4] table slots per workgroup. */
int pcp_view_pair_stats(pcp_context *ctx, uint64_t *out_n, uint64_t *out_sum);
int pcp_view_pair_stats_counters(pcp_context *ctx, int64_t out[5]);
/* Host only, no context, no GPU: the gains of Brown & Lowe's gain compensation from the pair matrices.  Keyframes without
 * a pair get exactly 1.0; the others minimise
 *   sum_i sum_j n_ij [ (g_i I_ij - g_j I_ji)^2 / sigma_n^2 + (1 - g_i)^2 / sigma_g^2 ],   I_ij = sum_ij / n_ij  (fp64),
 * a symmetric positive definite linear system solved by a dense fp64 Cholesky in a fixed order (deterministic; O(F^3)).
 * sigma_n in luma levels (10 is the usual choice), sigma_g the prior's width (0.1).  The diagonal of the matrices is not read.
 * PCP_ERR_INVALID: n_frames < 1, a NULL argument, a sigma that is not finite and positive, n not symmetric, or
 * sum_ij > 255 n_ij.  PCP_ERR_RANGE: n_frames > 4096.  The message is at pcp_last_error(NULL). */
int pcp_exposure_gains(int32_t n_frames, const uint64_t *n, const uint64_t *sum, double sigma_n, double sigma_g, double *out_gains);
/* gains == NULL: off.  Otherwise n must be the keyframe count and every gain finite and in (0, 16], else PCP_ERR_INVALID
 * and the setting is unchanged.  pcp_set_frames clears the gains.  While set, pcp_colour_finalise replaces every listed
 * view's channel c by  c' = min((int)(fl32(fl32(c) * (float)g_f) + 0.5f), 255)  (fp32, no fusion, the cast truncates) and
 * then runs its own arithmetic on c' (fp32 sums in list order, division, truncation, has = (r | g | b) != 0): out_rgb,
 * out_has, the packed result and everything that reads it (pcp_colour_compact*, pcp_colour_smooth_local,
 * pcp_download_result_packed*).  All gains 1.0 give the bits of a run without gains.  out_top_rgb / out_top_score /
 * out_top_frame / out_count and the fused labels stay raw.  pcp_colorize and pcp_colorize_from_depth return PCP_ERR_STATE
 * while gains are set: their kernels keep the lists in registers; use pcp_colour_reset / pcp_colour_pass /
 * pcp_colour_finalise. */
int pcp_set_frame_gains(pcp_context *ctx, const double *gains, int32_t n);

/* PointCloudProcessor::smoothColorsWithLocalRegion(rgbCloud, radius), PointCloudProcessor.cpp:634-703, whose call
 * smoothColorsWithLocalRegion(rgbCloud, 0.1) is commented out at :597 between smoothColors (:596) and
 * removePointsWithNoColor (:598): an opt-in post-pass over the finished colours.  Every finite point
 * takes floor(sum w_j c_j / sum w_j) per channel over the finite points j with fl32 squared distance <= radius^2 (itself
 * included), w_j = fl32(1 / (1 + d2)); the sums are exact (integer weights w_j * 2^24), so the result is bit-reproducible.
 * Every output reads the unsmoothed colours; has = (r | g | b) != 0 afterwards; non-finite points keep their word.
 * radius must be finite with 0 < radius <= 1 (else PCP_ERR_INVALID).  *out_has_count (nullable) = points with has set.
 * The pass builds the smoothing stages' grid: an open pcp_mls_stream_* / pcp_cloud_smooth_stream_* / pcp_sor_partial
 * state of the context ends (as with any call that builds it).
 * In place on the context's colour result (valid after pcp_colour_finalise / pcp_colorize / pcp_colorize_from_depth, else
 * PCP_ERR_STATE); later pcp_download_result_packed[_async] / pcp_colour_result_device return the smoothed words.  The
 * top-5 lists of pcp_colour_finalise are not touched.  The result moves to the other half of the double buffer: an
 * asynchronous download still in flight keeps reading the unsmoothed words. */
int pcp_colour_smooth_local(pcp_context *ctx, float radius, int64_t *out_has_count);
/* The same over caller-supplied packed words r | g<<8 | b<<16 | has<<24 (n = pcp_cloud_size; the has bit of the input is
 * not read), host memory or device memory of the context's GPU; in == out allowed.  Synchronous. */
int pcp_colour_smooth_local_packed(pcp_context *ctx, float radius, const uint32_t *in_rgba, uint32_t *out_rgba,
                                   int64_t *out_has_count);

/* ---- MLS (CloudSmooth::process, PCP/src/cloudSmooth.cpp:77-185) ---------- */
/* pcl::MovingLeastSquares on the uploaded cloud (radius search + order-2 fit +
 * SIMPLE projection; upsampling NONE, SAMPLE_LOCAL_PLANE or VOXEL_GRID_DILATION).  Results stay on
 * the device; *out_count = number of output points.
 * SAMPLE_LOCAL_PLANE: every fitted point (>= 3 neighbours) emits one row per sample (u, v) of the table
 * pcp_mls_local_plane_samples returns for the context's (radius, step), in table order, projected onto its fitted
 * polynomial (the plane when the polynomial was not fitted); rows grouped by source point in ascending input index.
 * Rows = table size x fitted points, < 2^31 and within device memory, else PCP_ERR_NOMEM before any row is allocated. */
int pcp_mls_process(pcp_context *ctx, const pcp_mls_params *p, int64_t *out_count);
/* SAMPLE_LOCAL_PLANE's upsampling_radius / upsampling_step (MLSParameters slp_upsampling_radius / _stepsize,
 * cloudSmooth.hpp:28-29; the reference sets 0.05 / 0.01, PointCloudProcessor.cpp:74-75, which pcp_create sets too).
 * Both finite and > 0, radius / step <= PCP_MLS_SLP_MAX_RATIO, and both representable as positive finite floats;
 * else PCP_ERR_INVALID and the setting is unchanged. */
int pcp_set_mls_local_plane(pcp_context *ctx, double upsampling_radius, double upsampling_step);
/* The SAMPLE_LOCAL_PLANE table, host only (no context, no GPU): MovingLeastSquares::computeMLSPointNormal's loop
 *   for (float u = -(float)R; u <= R; u += (float)S) for (float v = -(float)R; v <= R; v += (float)S)
 *     if (u * u + v * v < R * R) emit(u, v)
 * restated exactly (fp32 products and sum without fusion, compared in double) [upstream].  The table is neither the
 * integer lattice nor symmetric: (0.05, 0.01) gives 79 samples.  *out_count = the table's size; up to `capacity`
 * samples go to out_u / out_v (either nullable) in emission order.  Arguments as pcp_set_mls_local_plane, else
 * PCP_ERR_INVALID. */
int pcp_mls_local_plane_samples(double radius, double step, int64_t capacity, float *out_u, float *out_v, int64_t *out_count);
/* Multi-GPU form: the whole cloud is uploaded on every rank and this rank fits
 * only the queries index_begin <= i < index_end (upsampling NONE).  Outputs as pcp_mls_process. */
int pcp_mls_process_shard(pcp_context *ctx, const pcp_mls_params *p, int64_t index_begin, int64_t index_end,
                          int64_t *out_count);
/* The same deal by SLABS of the stage's own spatial order (consecutive places of its cell-sorted cloud, whole wavefronts):
 * slab `slab` of `n_slabs` is 1 / n_slabs of the work whatever order the caller's points come in (an index range only
 * divides the work when the caller's order is spatially coherent).  Outputs as pcp_mls_process: the slab's rows in input
 * order; the slabs' results merged by source index are the unsharded result. */
int pcp_mls_process_slab(pcp_context *ctx, const pcp_mls_params *p, int32_t slab, int32_t n_slabs, int64_t *out_count);
/* VOXEL_GRID_DILATION in chunks.  One result holds fewer than 2^31 points and must fit the device (78 B per point); the
 * reference's own configuration (1 mm voxels, 4 dilations, PointCloudProcessor.cpp:78-81) turns every input point into up
 * to 729 output points -- ~3.8e9 for a 10 M-point map -- and pcp_mls_process then fails with PCP_ERR_NOMEM.  The
 * streamed form fits the surfaces once, counts the dilated voxel set in 64 bits (*out_total) and cuts its ascending key
 * order into *out_chunks chunks of at most chunk_capacity voxels; every pcp_mls_stream_next emits the next chunk into
 * the result buffers (read with pcp_mls_fetch; *out_count = its points, 0 after the last chunk).  The chunks in order
 * are exactly what one pcp_mls_process would return.  No other call on ctx may come between begin and the last next. */
int pcp_mls_stream_begin(pcp_context *ctx, const pcp_mls_params *p, int64_t chunk_capacity, int64_t *out_total,
                         int32_t *out_chunks);
int pcp_mls_stream_next(pcp_context *ctx, int64_t *out_count);
/* The chunk the next pcp_mls_stream_next emits (0 .. chunks; a chunk may be emitted more than once): several GPUs that
 * hold the same cloud and began the same stream deal the chunks out among themselves (chunk c to GPU c mod N). */
int pcp_mls_stream_seek(pcp_context *ctx, int32_t chunk);
/* xyz / normal 3*m floats AoS, curvature m, source index m (input order for
 * NONE; ascending voxel key for VOXEL_GRID_DILATION). */
int pcp_mls_fetch(pcp_context *ctx, int64_t capacity, float *out_xyz, float *out_normal, float *out_curvature,
                  int32_t *out_index);
/* CloudSmooth::process end to end on the device: SOR(sor_mean_k, sor_std_mul) ->
 * MovingLeastSquares (+ upsampling) -> SOR, cloudSmooth.cpp:109-164.  Results through
 * pcp_mls_fetch; out_index refers to the uploaded cloud.
 * SAMPLE_LOCAL_PLANE: the fit runs on the first filter's survivors exactly as pcp_mls_process runs on an upload of them
 * (ascending input index, the same grids), so the rows before the last filter are that call's rows bit for bit; the
 * survivors of the last filter keep that row order.  The last filter's cost grows with rows x rows thrown off their surface
 * by broken fits, so the chain refuses with PCP_ERR_RANGE, before that filter runs, more than 2^24 rows, and rows whose box
 * would force the filter's grid cells beyond 2 * step * sqrt((sor_mean_k + 1) / pi).  The query sharding (_shard, _slab) and the streamed forms
 * (pcp_mls_stream_begin, pcp_cloud_smooth_stream_begin) refuse SAMPLE_LOCAL_PLANE with PCP_ERR_INVALID. */
int pcp_cloud_smooth(pcp_context *ctx, const pcp_mls_params *p, int64_t *out_count);

/* CloudSmooth::process WHOLE for clouds whose dilated voxel set exceeds one result (PCP/src/cloudSmooth.cpp:109-164 with the
 * reference's own MLS configuration, PointCloudProcessor.cpp:67-86: VOXEL_GRID_DILATION 1 mm x 4 makes ~3.8e9 points of a
 * 10 M-point map): StatisticalOutlierRemoval -> MovingLeastSquares + upsampling -> StatisticalOutlierRemoval ON THE UPSAMPLED
 * CLOUD (:160-164), the last two stages streamed over chunks of the voxel key order (whole planes of the first axis).
 *   _begin: first filter, fit, voxel set; sweep 0 projects a sample of the voxels to size the halo; then sweep 1 -- every chunk
 *           is emitted together with a halo of neighbouring planes, the mean k-NN distances of its own rows are computed against
 *           chunk + halo and kept on the device (4 B per row of the whole upsampled cloud), (sum, sum of squares) are taken over
 *           ALL rows in row order, the filter's threshold follows.  The halo is CHECKED, not assumed: a row's neighbourhood (bound
 *           of the distance to its (k + 1)-th nearest) must end inside the part of space whose rows the halo is guaranteed to
 *           hold, given the largest displacement any row has from its voxel (taken over every row sweep 1 emitted -- all of them);
 *           a chunk that fails is redone with a wider halo.  The distances are therefore the ones the one-shot pcp_cloud_smooth
 *           computes, bit for bit; the threshold is summed in another order (row order instead of the cell order of one big
 *           grid) and agrees to rounding (~1e-16 relative).
 *           out_total_rows = rows of the upsampled cloud before the last filter, out_kept_rows = after it.
 *   _next:  sweep 2 -- the next chunk's own rows are emitted again, classified by their stored distance and compacted:
 *           *out_count survivors in key order, fetched with pcp_mls_fetch (out_index refers to the uploaded cloud); 0 after
 *           the last chunk.  The concatenation over the chunks is what pcp_cloud_smooth returns when the cloud fits one result.
 *   _end:   ends the stream and frees the distances (4 B per row: 11 GB for a 10 M-point map).  Optional: the next stream of
 *           the context reuses them, a one-shot upsampling call that would not fit without them takes them, pcp_destroy frees them.
 * chunk_capacity: most voxels per chunk, own rows (>= 4096; every plane of the voxel grid must fit). */
int pcp_cloud_smooth_stream_begin(pcp_context *ctx, const pcp_mls_params *p, int64_t chunk_capacity, int64_t *out_total_rows,
                                  int64_t *out_kept_rows, int32_t *out_chunks);
int pcp_cloud_smooth_stream_next(pcp_context *ctx, int64_t *out_count);
int pcp_cloud_smooth_stream_end(pcp_context *ctx);
/* The chunk the next pcp_cloud_smooth_stream_next emits, 0 <= chunk <= chunks (else PCP_ERR_RANGE); with chunk == chunks that
 * call returns 0 rows.  Sweep 2 reads stored distances, so a chunk may be emitted any number of times: the stream stays open
 * after its last chunk until _end, an upload or another smoothing call ends it.  No open stream: PCP_ERR_STATE. */
int pcp_cloud_smooth_stream_seek(pcp_context *ctx, int32_t chunk);
/* diagnostic of the last pcp_cloud_smooth_stream_begin: out[0] halo in planes (as finally used, the widest), [1] chunks redone
 * with a wider halo, [2] threshold of the last filter, [3] largest |x displacement| of a row from its voxel (m; over all rows),
 * [4] smallest margin of any chunk (m; > [3] proves the halo), [5] rows computed including halos, [6] the displacement sweep 0's
 * sample saw (m; sized the halo), [7] bytes of device memory the stream holds at the time of the call, [8..11] host-clock
 * seconds of _begin: first filter + fit + voxel set, [9] device allocations (hipMalloc / hipFree: they lie inside the other
 * three; seconds on a first call, none afterwards), sweep 0, sweep 1 + threshold, [12] bytes allocated during _begin. */
int pcp_cloud_smooth_stream_stats(pcp_context *ctx, double out[13]);
/* pcl::StatisticalOutlierRemoval (k, std_mul) keep mask of the uploaded cloud,
 * cloudSmooth.cpp:109-116,160-164.
 * The smoothing entry points (pcp_sor, pcp_mls_process[_shard], pcp_cloud_smooth, pcp_close_pairs) need finite
 * coordinates: a cloud with NaN or infinite points is refused with PCP_ERR_INVALID (PCL's filters skip such points one
 * by one; the projection / colour entry points accept them and reject the points, Appendix B6). */
int pcp_sor(pcp_context *ctx, int32_t mean_k, double std_mul, uint8_t *out_keep, int64_t *out_kept);
/* Multi-GPU form of pcp_sor (the cloud on every GPU, the queries dealt out).  The queries are dealt out by
 * SLABS of the filter's own spatial order (consecutive places of its cell-sorted cloud), not by the caller's indices: a
 * wavefront holds 64 consecutive places, so a slab is whole wavefronts and 1 / n_slabs of the work whatever order the
 * caller's points come in.  The filter's threshold is mean + std_mul * stddev of ALL mean distances (cloudSmooth.cpp:113-115 ->
 * statistical_outlier_removal.hpp [upstream]), so a slab cannot classify alone; the statistics are kept as one (sum, sum of
 * squares) pair per chunk of pcp_sor_chunk_points() consecutive places, each chunk summed in a fixed order by the GPU whose
 * slab holds it (slabs are whole chunks):
 *   pcp_sor_partial  mean distances of slab `slab` of `n_slabs` and its chunk sums: 2 doubles per chunk into out_chunk_sums,
 *                    *out_first_chunk / *out_chunks = where they belong among the ceil(n / chunk) pairs of the cloud;
 *   (the caller puts the slabs' arrays together: the array one GPU computes)
 *   pcp_sor_finish   threshold from all chunk sums, keep flags of the slab's points: out_keep[i] (n bytes, the caller's
 *                    indices, 0 for every point of another slab -- the OR of the slabs' arrays is the filter's mask).
 * pcp_sor itself is partial + finish with one slab: the sharded keep mask equals it bit for bit. */
int64_t pcp_sor_chunk_points(void);
int pcp_sor_partial(pcp_context *ctx, int32_t mean_k, int32_t slab, int32_t n_slabs, int64_t capacity, double *out_chunk_sums,
                    int64_t *out_first_chunk, int64_t *out_chunks);
int pcp_sor_finish(pcp_context *ctx, double std_mul, const double *all_chunk_sums, int64_t n_chunks, int32_t slab, int32_t n_slabs,
                   uint8_t *out_keep, int64_t *out_kept);

/* ---- NID extrinsic refinement (VisualLiDARCalibration::calibrate, PCP/src/calibrate.cpp:42-126) -- */
/* per-point intensity of the uploaded cloud (pcl::PointXYZI::intensity), needed by the NID stage */
int pcp_upload_intensity(pcp_context *ctx, const float *intensity, int64_t n);
/* Builds every keyframe's NID input on the device: its z-buffer-culled points in camera
 * coordinates with intensity (the content of <ts>_beforeNID.pcd, PointCloudProcessor.cpp:178-224).
 * Needs camera, cloud, intensity, keyframes and images.
 * Repeat it after pcp_set_camera, pcp_set_frames, any pcp_upload_cloud* and pcp_upload_intensity: each of them drops what
 * it built, and the pcp_nid_* calls below then return PCP_ERR_STATE.  The images are read at every evaluation: a
 * pcp_upload_image* after it needs no repeat. */
int pcp_nid_prepare(pcp_context *ctx, int64_t *out_points);
/* MultiNIDCost at T = T_camera_lidar (4x4 row-major fp64): sum over keyframes of NIDCost
 * (nid_cost.hpp:42-116), and its gradient in the SE(3) tangent of T * exp(delta),
 * delta = (upsilon, omega).  T_init (nullable): the initial guess whose +-0.2 m / 2 deg
 * neighbourhood bounds the domain (visual_camera_calibration.cpp:100-105); outside it, or when
 * a keyframe's cost is not finite, *valid = 0. */
int pcp_nid_evaluate(pcp_context *ctx, const double T[16], const double *T_init, int32_t bins, double *cost,
                     double grad6[6], int32_t *valid);
/* VisualCameraCalibration::calibrate (visual_camera_calibration.cpp:49-80): up to
 * max_outer_iterations runs of a BFGS minimisation on SE(3) (stands in for ceres::Solve),
 * stopping when the pose moves by < 1 cm and < 1 deg.  T_out feeds pcp_set_frames' T_opt. */
int pcp_nid_optimize(pcp_context *ctx, const double T_init[16], int32_t bins, int32_t max_outer_iterations,
                     double T_out[16], double *final_cost, int32_t *evaluations);

/* The same cost over an index-sharded map (one context per GPU, each holding a slice of the cloud and of the
 * intensities; keyframes and images replicated; depth maps MIN-merged, PCP_DEPTH_BATCHED).  A keyframe's joint histogram
 * (nid_cost.hpp:55-93) is a sum over its points, so: every shard accumulates its own histograms at T
 * (pcp_nid_accumulate), the shards' histograms are added in place -- an all-reduce(SUM) over the `count` doubles at
 * pcp_nid_histograms_device, queued on the context's stream or completed before the next call -- and pcp_nid_finish
 * turns the summed histograms into cost and gradient, the same numbers on every shard.  On one context
 * pcp_nid_evaluate == pcp_nid_accumulate + pcp_nid_finish (plus the domain test against T_init). */
int pcp_nid_accumulate(pcp_context *ctx, const double T[16], int32_t bins);
int pcp_nid_histograms_device(pcp_context *ctx, void **device_ptr, int64_t *count);
int pcp_nid_finish(pcp_context *ctx, int32_t bins, double *cost, double grad6[6], int32_t *valid);
/* pcp_nid_optimize with the cost supplied by the caller (the sharded evaluation above, driven by the host that owns the
 * shards): eval returns PCP_OK and fills cost / grad6 / valid for a T inside the domain; the loop, its tolerances and the
 * domain test are those of pcp_nid_optimize.  ctx only carries the error text. */
typedef int (*pcp_nid_eval_fn)(void *user, const double T[16], int32_t bins, double *cost, double grad6[6], int32_t *valid);
int pcp_nid_optimize_with(pcp_context *ctx, pcp_nid_eval_fn eval, void *user, const double T_init[16], int32_t bins,
                          int32_t max_outer_iterations, double T_out[16], double *final_cost, int32_t *evaluations);

/* ---- device PCD writer (pcl::PCDWriter::writeASCII, every file the program hands out) --------------------- */
/* The rows of the ASCII PCD files as text, formatted on the device and downloaded as the bytes that follow the header
 * ("Device PCD writer"): floats as "%.8g" of the fp32 (ostream precision 8; every NaN prints "nan"), the rgb
 * column as the packed word 0xff000000 | r<<16 | g<<8 | b and segmentMask as "%u", single spaces, one '\n' per row --
 * byte for byte what host/pcd_io.hpp's writeASCII_* print.  Opt-in: nothing runs unless one of these is called; a caller
 * detects support by the symbols (PCP_ABI_VERSION is unchanged). */
#define PCP_ROWS_XYZI 0        /* x y z intensity                  savePCDFileASCII :135 (scans-crop.pcd), writeASCII :217 (_beforeNID.pcd) */
#define PCP_ROWS_XYZRGB 1      /* x y z rgb                        writeASCII :920 (cloudInWorldWithRGB.pcd) */
#define PCP_ROWS_XYZRGBMASK 2  /* x y z rgb segmentMask            writeASCII :542 (_rgb-mask.pcd), :936-954 (cloudInWorldWithRGBandMask.pcd) */
#define PCP_ROWS_POINTNORMAL 3 /* x y z nx ny nz curvature         pcl::io::savePCDFile, cloudSmooth.cpp:180-181 (<stem>_mls.pcd) */
/* longest row of a kind in bytes, newline included (60 / 56 / 62 / 105); <0 for an unknown kind.  Host only. */
int64_t pcp_ascii_row_bound(int32_t kind);
/* Host only, no context, no GPU: the formatter the kernels use (csrc/pcp_ascii.hpp), run on the CPU -- the way to check it
 * on every bit pattern.  n rows: f row-major with 4 | 3 | 3 | 7 floats per row (kind order above), rgb 3 bytes per row
 * (r, g, b; the RGB kinds), mask one uint16 per row (XYZRGBMASK); arrays a kind does not read may be NULL.
 * *out_bytes (nullable) = the exact byte count of the n rows, always.  capacity below it: PCP_ERR_RANGE and out_text is
 * left untouched (size the buffer as n * pcp_ascii_row_bound(kind), or call again with the reported count).  Negative n
 * or capacity, an unknown kind, a missing array: PCP_ERR_INVALID.  n == 0: 0 bytes, PCP_OK.  The message of a failure is
 * at pcp_last_error(NULL). */
int pcp_ascii_rows_host(int32_t kind, int64_t n, const float *f, const uint8_t *rgb, const uint16_t *mask, int64_t capacity,
                        char *out_text, int64_t *out_bytes);
/* The same rows formatted on the device from host arrays (the sites that hold their rows on the host: scans-crop.pcd :135,
 * the per-keyframe dumps :217 and :542).  Same arguments and rules; out_text is host memory, pageable or pinned, and is not
 * retained.  Synchronous. */
int pcp_ascii_rows(pcp_context *ctx, int32_t kind, int64_t n, const float *f, const uint8_t *rgb, const uint16_t *mask,
                   int64_t capacity, char *out_text, int64_t *out_bytes);
/* Rows [first_row, first_row + max_rows) of what pcp_colour_compact would return -- removePointsWithNoColor's survivors
 * (:598), the final files :917-920 / :936-954 -- as XYZRGB text, or XYZRGBMASK text with the fused label as segmentMask
 * (with_label != 0).  The kernels read the compaction's index list, the uploaded planes, the packed colour word and the
 * labels in place; no binary row is materialised.  *out_rows = rows in the window (0 past the end), *out_bytes = their exact
 * byte count; capacity rules as above.  No colour result, or with_label on a result made without label fusion:
 * PCP_ERR_STATE.  Negative first_row / max_rows / capacity: PCP_ERR_INVALID.  Every call takes the compaction again. */
int pcp_colour_compact_ascii(pcp_context *ctx, int32_t with_label, int64_t first_row, int64_t max_rows, int64_t capacity,
                             char *out_text, int64_t *out_rows, int64_t *out_bytes);
/* Rows [first_row, first_row + max_rows) of what pcp_mls_fetch would return (xyz, normal, curvature of the latest smoothing
 * result or stream chunk), as POINTNORMAL text (<stem>_mls.pcd, cloudSmooth.cpp:180-181).  Same rules. */
int pcp_mls_fetch_ascii(pcp_context *ctx, int64_t first_row, int64_t max_rows, int64_t capacity, char *out_text,
                        int64_t *out_rows, int64_t *out_bytes);

/* ---- device PCD reader (pcl::io::loadPCDFile of a DATA ascii file: PointCloudProcessor.cpp:112, :148, cloudSmooth.cpp:92) - */
/* The x y z intensity floats of a window of PCD ASCII rows ("Device PCD reader", DR1-DR8): every value bit for bit
 * what glibc's strtof returns for its token -- the fp32 nearest the exact decimal value, ties to even, computed on integers --
 * and so what host/pcd_io.hpp's loadPCDFile returns.  A row ends at '\n'; tokens are separated by space \t \r \v \f; a row
 * needs `columns` tokens (more are ignored); only the tokens of the columns read are examined, and they must be
 * [+-]? (D+ ('.' D*)? | '.' D+) ([eE] [+-]? D+)? with at most 19 digits between the first and the last non-zero digit of the
 * significand and at most 5 exponent digits, or nan / inf / infinity in any case with an optional sign.  Every other row is
 * BAD (too few tokens, blank, hex floats, "1.5abc", NUL bytes, 20 significant digits, ...), and so is a row of more than
 * PCP_ASCII_PARSE_MAX_ROW bytes in front of its '\n'.  A bad row is never given a value: the caller hands such a file to
 * its own reader.  Opt-in: nothing runs unless called; PCP_ABI_VERSION is unchanged, a caller detects support by the symbols. */
#define PCP_ASCII_PARSE_MAX_ROW 65536 /* bytes of a row in front of its '\n' */
/* pcp_ascii_parse_limit(which): the sizes the implementation works with (the tests place rows around them); <0: unknown */
#define PCP_PARSE_LIMIT_ROW 0       /* PCP_ASCII_PARSE_MAX_ROW */
#define PCP_PARSE_LIMIT_TILE 1      /* bytes of text a workgroup stages into LDS; a longer span is walked in global memory */
#define PCP_PARSE_LIMIT_PIECE 2     /* bytes per upload piece of a window */
#define PCP_PARSE_LIMIT_TILE_ROWS 3 /* rows per workgroup */
#define PCP_PARSE_LIMIT_WINDOW 4    /* bytes per call: 2^31 - 1 (row offsets are 32-bit); a longer window is PCP_ERR_RANGE */
int64_t pcp_ascii_parse_limit(int32_t which);
/* Host only, no context, no GPU: the parser the kernels use (csrc/pcp_ascii_parse.hpp), run on the CPU -- the way to check it on
 * every bit pattern.  The window is text[0, bytes).  columns: scalars per row (sum of COUNT).  col[0..3]: 0-based column of x,
 * y, z, intensity; col[3] = -1: none (0.0f).  The bytes after the last '\n' are a row only when final_window != 0 and they
 * hold a non-blank byte; otherwise they stay unconsumed for the caller's next window.
 * *out_rows = rows parsed: the smallest of max_rows, the rows of the window and the index of the first bad row; out_x / _y /
 * _z / _intensity [0, *out_rows) are written, the entries behind them left untouched.  *out_consumed = the offset just past
 * the last parsed row (the start of the bad row when one ends the parse).  *out_bad_row = -1 or the index of the first bad
 * row; a bad row is not an error (PCP_OK).  NULL outputs, negative bytes or max_rows, columns outside 1..64, a col entry
 * outside -1..columns-1 (-1 for the intensity only): PCP_ERR_INVALID.  bytes above 2^31 - 1: PCP_ERR_RANGE.  bytes == 0: 0
 * rows, PCP_OK.  The message of a failure is at pcp_last_error(NULL). */
int pcp_ascii_parse_host(const char *text, int64_t bytes, int32_t columns, const int32_t col[4], int32_t final_window,
                         int64_t max_rows, float *out_x, float *out_y, float *out_z, float *out_intensity,
                         int64_t *out_rows, int64_t *out_consumed, int64_t *out_bad_row);
/* The same window parsed on the device: same arguments, same results.  text and the outputs are host memory, pageable or
 * pinned, and are not retained; the window goes up in pieces through pinned staging while the kernels of the piece before
 * run and the rows of the one before that come down.  Synchronous.  Kernels are timed under PCP_K_MISC. */
int pcp_ascii_parse(pcp_context *ctx, const char *text, int64_t bytes, int32_t columns, const int32_t col[4], int32_t final_window,
                    int64_t max_rows, float *out_x, float *out_y, float *out_z, float *out_intensity,
                    int64_t *out_rows, int64_t *out_consumed, int64_t *out_bad_row);

/* ---- voxel-grid output (pcl::VoxelGrid on the final files; voxelgrid_sampling, PCP/src/vlcal/common/frame_cpu.cpp:360-451) - */
/* One row per occupied voxel of edge `leaf` -- centroid, mean colour, mean fused label, row count -- accumulated on the
 * device over any number of colour results: one-shot runs, index shards, the chunks of a streamed cloud (DESIGN.md,
 * "Voxel-grid output", VG1-VG7).  The rows that enter are those pcp_colour_compact returns (has bit set; after
 * pcp_colour_smooth_local the smoothed ones), with the uploaded coordinates.  Exact integers throughout, so the result does
 * not depend on the order of rows, uploads or atomics:
 *   leaf      fp32, 1e-4 <= leaf <= 1 (else PCP_ERR_INVALID); inv = f32(1.0f / leaf);
 *   cell      c = (int32)floorf(f32(x * inv)) per axis: the lattice is anchored at the world origin, so shards and chunks
 *             agree; a non-finite coordinate or |c| >= 2^20 is PCP_ERR_RANGE;
 *   order     ascending key ((cz + 2^20) << 42) | ((cy + 2^20) << 21) | (cx + 2^20): x fastest, z slowest;
 *   position  signed 64-bit sum of q = llrint((double)x * 2^32) - corner, corner = llrint((double)c * (double)leaf * 2^32);
 *             x_out = f32((double)(corner + floor((2 * sum q + n) / (2 n))) * 2^-32);
 *   colour    r_out = floor(sum r / n), likewise g, b and the label; count = n.  A voxel with n >= 2^24: finish returns
 *             PCP_ERR_RANGE.
 * A voxel of one row with |x| >= 2^-9 returns that coordinate bit for bit.  Opt-in: nothing runs unless one of these is
 * called, PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.
 *
 * The accumulator belongs to the context: it outlives pcp_upload_cloud*, pcp_upload_cloud_from_result, pcp_colour_reset,
 * pcp_set_frames and pcp_set_camera; only _begin, _end and pcp_destroy drop it.  The sums are local to the context (on an
 * index shard: to the shard); exchanging them across GPUs is the caller's.
 * _begin  starts an empty accumulation (dropping a previous one).  initial_slots: slots of the hash table (rounded up to a
 *         power of two, at least 64; at most 2^31), 0 = sized by the first add; the table doubles as it fills past a half.
 * _add    adds the rows of the current colour result; *out_rows_added (nullable) = their number.  Needs _begin
 *         (PCP_ERR_STATE), a live colour result (PCP_ERR_STATE), and no _finish since _begin (PCP_ERR_STATE).  The first add
 *         fixes whether labels are accumulated, by whether its result was made with label fusion; a later add that disagrees
 *         is PCP_ERR_STATE.  A failed add leaves the accumulation as it was.  It changes nothing else: the packed colour
 *         words and pcp_colour_compact's rows are afterwards what they were before.
 * _finish sorts the occupied voxels by key and computes the rows; *out_voxels (nullable) = their number.  A second call
 *         returns the same count.
 * _fetch  rows [first, first + max_rows) of the finished result, every output nullable: out_xyz 3 floats, out_rgb 3 bytes
 *         (r, g, b), out_label and out_count one each per row; *out_rows = rows in the window (0 past the end).  Before
 *         _finish, or out_label on an accumulation without labels: PCP_ERR_STATE.  Negative first / max_rows: PCP_ERR_INVALID.
 * _stats  out[0..5] = rows added, voxels (before _finish: keys that hold rows), table slots, table doublings, per-wavefront
 *         partial sums issued, global payload adds issued (7 per partial, 8 with labels).  Before _begin: PCP_ERR_STATE.
 * _end    drops the accumulation and its result. */
int pcp_voxel_reduce_begin(pcp_context *ctx, float leaf, int64_t initial_slots);
int pcp_voxel_reduce_add(pcp_context *ctx, int64_t *out_rows_added);
int pcp_voxel_reduce_finish(pcp_context *ctx, int64_t *out_voxels);
int pcp_voxel_reduce_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, float *out_xyz, uint8_t *out_rgb, uint8_t *out_label,
                           uint32_t *out_count, int64_t *out_rows);
int pcp_voxel_reduce_stats(pcp_context *ctx, int64_t out[6]);
int pcp_voxel_reduce_end(pcp_context *ctx);
/* Host only, no context, no GPU: the same reduction of n rows (xyz 3 floats, rgb 3 bytes, label one byte per row; label
 * nullable: the labels then read 0) by the arithmetic the kernels use (csrc/pcp_voxel_reduce.hpp).  *out_voxels = the occupied
 * voxels, always; the first min(capacity, voxels) rows are written (outputs nullable).  Leaf and range rules as above; negative
 * n / capacity, a missing xyz / rgb, out_label without label: PCP_ERR_INVALID.  The message is at pcp_last_error(NULL). */
int pcp_voxel_reduce_host(float leaf, int64_t n, const float *xyz, const uint8_t *rgb, const uint8_t *label, int64_t capacity,
                          float *out_xyz, uint8_t *out_rgb, uint8_t *out_label, uint32_t *out_count, int64_t *out_voxels);

/* ---- orthographic maps (no counterpart in the reference, which stops at per-keyframe perspective pictures: ------------- */
/* ---- scripts/genNormAndDistanceMask.py visualize_skeleton_edge_pts, save_results) ----------------------------------- */
/* One metric picture of the coloured cloud -- colour, depth, point index, fused label at a fixed number of metres per pixel
 * -- accumulated on the device over any number of colour results: one-shot runs, the chunks of a streamed cloud (DESIGN.md,
 * "Orthographic maps", OM1-OM8).  Opt-in: nothing runs unless one of these is called, PCP_ABI_VERSION is unchanged and a
 * caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.
 *   frame     origin o, axes u (image x, to the right), v (image y, down), n (viewing direction, into the scene), gsd in
 *             metres per pixel (1e-4 <= gsd <= 1; inv = f32(1.0f / gsd)), width and height in 1..16384 with width * height
 *             <= 2^26, a depth window d_min < d_max.  A non-finite value, a gsd outside its range, an empty raster or window,
 *             or axes that are not orthonormal and right-handed (u x v = n) within 1e-3: PCP_ERR_INVALID.  A raster past the
 *             limits: PCP_ERR_RANGE, and the message names the gsd at which the same extent fits.
 *   point     fp32, every operation rounded: d = p - o; s = d.u, t = d.v, depth = d.n with d.c = dx*cx + (dy*cy + dz*cz);
 *             a = s * inv, b = t * inv.  A row contributes iff its has bit is set, its coordinates are finite,
 *             0 <= a < (float)width, 0 <= b < (float)height (compared in float) and d_min <= depth <= d_max; its pixel is
 *             (int32)floorf(b) * width + (int32)floorf(a).  A depth of -0 counts as +0.
 *   winner    per pixel the contributor with the smallest depth, ties to the lowest GLOBAL index g = index_base + row.  Because
 *             the global index is part of the comparison the result does not depend on the order of the adds, of the rows or
 *             of the atomics: a cloud added in pieces gives the bytes of the same cloud added at once.  The global index
 *             ranges of the adds must be DISJOINT; two rows with one global index give one of their payloads, unspecified
 *             which.  index_base < 0 or index_base + pcp_cloud_size > 2^32 - 1: PCP_ERR_RANGE.
 * The accumulator (12 B per pixel) belongs to the context: it outlives pcp_upload_cloud*, pcp_upload_cloud_from_result,
 * pcp_colour_reset, pcp_set_frames and pcp_set_camera; only _begin, _end and pcp_destroy drop it.
 * _begin      starts an empty map of the frame (dropping a previous one).
 * _add        adds the rows of the current colour result with the uploaded coordinates -- the rows pcp_colour_compact returns;
 *             *out_contributors (nullable) = the rows that fell inside the raster and the window.  Needs _begin, a live colour
 *             result and no _finish since _begin (each PCP_ERR_STATE).  The first add fixes whether labels are held, by
 *             whether its result was made with label fusion; a later add that disagrees is PCP_ERR_STATE.  A failed add leaves
 *             the map as it was.  It changes nothing else: the packed colour words and pcp_colour_compact's rows are
 *             afterwards what they were before.
 * _add_packed the same for pcp_cloud_size words r | g<<8 | b<<16 | has<<24 of the caller's, in host memory or device memory of
 *             the context's GPU, over the uploaded cloud (no colour result needed): a layer that is not the colour, e.g. a
 *             width heat map.  The label is 0; it counts as an add without labels.
 * _finish     fill_radius_px R in 0..1024 (else PCP_ERR_INVALID).  R = 0: the map is what the adds left.  R > 0: an empty pixel
 *             whose nearest occupied pixel lies within d2 <= R^2 (the exact distance transform of pcp_mask_edt with the
 *             occupied pixels as its background; of several equally near pixels the one with the lowest linear index) takes
 *             that pixel's index, depth and payload.  *out_occupied, *out_filled (nullable) = pixels with a contributor of
 *             their own, pixels filled.  A map without an occupied pixel stays empty.  A second call returns the same counts
 *             (with another R: that R's); an add after a finish is PCP_ERR_STATE.  The fill's scratch (16 B per pixel) is freed
 *             on return; the source image (4 B per pixel) stays until _end.
 * _fetch      the layers, row-major height x width, every output a nullable host pointer: out_index uint32 global index
 *             (0xFFFFFFFF when empty), out_depth fp32 (0 when empty), out_rgb 3 bytes (r, g, b), out_label the fused label,
 *             out_status 0 empty / 1 direct / 2 filled, out_source int32 linear index of the pixel the values come from
 *             (itself when direct, -1 when empty).  Before _finish, or out_label on a map that holds no labels: PCP_ERR_STATE.
 * _stats      out[0..5] = contributors, atomics issued, occupied, filled (both as of the last _finish), adds, pixels.  Before
 *             _begin: PCP_ERR_STATE.
 * _end        drops the map. */
typedef struct pcp_ortho_frame {
  float o[3], u[3], v[3], n[3];
  float gsd;
  int32_t width, height;
  float d_min, d_max;
} pcp_ortho_frame;
int pcp_ortho_begin(pcp_context *ctx, const pcp_ortho_frame *frame);
int pcp_ortho_add(pcp_context *ctx, int64_t index_base, int64_t *out_contributors);
int pcp_ortho_add_packed(pcp_context *ctx, const uint32_t *rgba, int64_t index_base, int64_t *out_contributors);
int pcp_ortho_finish(pcp_context *ctx, int32_t fill_radius_px, int64_t *out_occupied, int64_t *out_filled);
int pcp_ortho_fetch(pcp_context *ctx, uint32_t *out_index, float *out_depth, uint8_t *out_rgb, uint8_t *out_label,
                    uint8_t *out_status, int32_t *out_source);
int pcp_ortho_stats(pcp_context *ctx, int64_t out[6]);
int pcp_ortho_end(pcp_context *ctx);
/* Host only, no context, no GPU: the same layers from n rows (xyz 3 floats, rgb 3 bytes; label and has one byte per row,
 * both nullable: label 0, every has bit set) with global indices index_base + row, by the arithmetic the kernels use
 * (csrc/pcp_ortho.hpp): a sequential minimum per pixel and pcp_mask_edt_host for the fill.  Outputs as _fetch's, all
 * nullable; the three counts as _add's and _finish's.  Frame, radius and index rules as above.  The message is at
 * pcp_last_error(NULL). */
int pcp_ortho_host(const pcp_ortho_frame *frame, int64_t n, const float *xyz, const uint8_t *rgb, const uint8_t *label,
                   const uint8_t *has, int64_t index_base, int32_t fill_radius_px, uint32_t *out_index, float *out_depth,
                   uint8_t *out_rgb, uint8_t *out_label, uint8_t *out_status, int32_t *out_source, int64_t *out_contributors,
                   int64_t *out_occupied, int64_t *out_filled);
/* Host only, fp64: a frame that looks straight at the rows with `has` set (NULL: all rows).  n is the eigenvector of the
 * smallest eigenvalue of their covariance (pcl::eigen33's closed form), signed so that `viewer` (3 doubles, e.g. the mean
 * camera centre) has negative depth -- with viewer NULL so that n's largest component is negative; u the eigenvector of the
 * largest eigenvalue with its largest component positive; v = n x u.  The origin lies on the fitted plane (the depth layer is
 * the relief off that plane), one pixel outside the rows' bounding rectangle; width and height are that rectangle plus two
 * pixels; d_min, d_max the rows' depth range widened by one gsd.  Every such row is a contributor of the frame.  Fewer than 3
 * rows, a gsd outside [1e-4, 1] or a non-finite result: PCP_ERR_INVALID; a size past the limits: PCP_ERR_RANGE, the gsd that
 * fits in the message (pcp_last_error(NULL)). */
int pcp_ortho_fit_frame_host(int64_t n, const float *xyz, const uint8_t *has, const double *viewer, float gsd, pcp_ortho_frame *out);

/* ---- orthophotos (no counterpart in the reference: scripts/genNormAndDistanceMask.py stops at per-keyframe pictures) ---- */
/* The finished orthographic map, walked at a finer pitch and coloured straight from the keyframe images: behind every fine
 * pixel a surface point (the map's depth, optionally interpolated), coloured by the rules the map points are coloured by --
 * projection, z-buffer keep rule against the context's depth maps, score, top-5 ("Orthophotos", OT1-OT9).  The mask
 * layer brings the keyframes' crack masks onto the metric raster at image resolution.  Opt-in: nothing runs unless called,
 * PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.  The kernel is timed under PCP_K_MISC.
 *   state     a live, finished map (pcp_ortho_finish); camera and keyframes set and every keyframe's image uploaded;
 *             PCP_CULL_ZBUFFER with the depth buffer on; every keyframe's depth map valid since the latest upload (the
 *             precondition of pcp_depth_accum_merge; after pcp_depth_accum_apply the merged maps count).  Else PCP_ERR_STATE,
 *             and the message names what is missing.  The call waits for pending image uploads and changes nothing it reads.
 *   raster    scale k in 1..16 fine pixels per ortho pixel and axis; the rectangle x0, y0, w, h in ORTHO pixels inside the map
 *             (w == 0 && h == 0 with x0 == y0 == 0: the whole map); views M in 1..5; max_step finite and > 0: else
 *             PCP_ERR_INVALID.  More than 2^28 fine pixels: PCP_ERR_RANGE, the message names the largest k that fits the
 *             rectangle.  More than 32 766 keyframes: PCP_ERR_RANGE.
 *   point     fine pixel (X, Y) of the output is (Xg, Yg) = (x0 k + X, y0 k + Y) of the whole fine raster; its parent is ortho
 *             pixel (Xg / k, Yg / k).  No source there: no surface.  Depth: the parent's, or with `interpolate` the bilinear
 *             depth between the parent and its neighbours towards the fine pixel (fp32, every operation rounded), taken only
 *             if every neighbour read lies inside the map, has a source and differs from the parent's depth by at most
 *             max_step.  Position: o + ((s u + t v) + d n) with s = ((float)Xg + 0.5f) * (gsd / (float)k), t alike.
 *   colour    keyframes ascending; a view is listed iff the point passes the keep rule and lies in the image; score as under
 *             PCP_MATCH_IDENTITY; sorted by descending score, ties to the lower keyframe.  The colour is the fp32 score-weighted
 *             mean of the first min(count, M) entries, truncated (M = 5: the reference's rule; M = 1: the sharpest).  With
 *             pcp_set_frame_gains in force every listed view's channels pass through the gain first.
 * Outputs, each a nullable host pointer, row-major (h k) x (w k): out_rgb 3 bytes (r, g, b); out_mask the mask byte of the best
 * view's texel (0 where that keyframe has no mask); out_status 0 no surface / 1 textured / 2 surface that no view lists;
 * out_view int16 keyframe of the best view (-1 when not textured); out_count min(listed views, 255); out_counts[0..3] = surface
 * pixels, textured, unseen, and the (tile of 16 x 16 fine pixels, keyframe) pairs the tile test skipped.  Pixels that are not
 * textured have rgb 0, mask 0, view -1.  Scratch: at most 8 B per fine pixel, freed on return. */
typedef struct pcp_ortho_texture_params {
  int32_t scale;        /* k: fine pixels per ortho pixel and axis, 1..16 */
  int32_t x0, y0, w, h; /* rectangle in ORTHO pixels; w == 0 && h == 0: the whole raster */
  int32_t views;        /* M: listed views that enter the colour, 1..5 (1 = sharpest, 5 = the reference's rule) */
  int32_t interpolate;  /* 0: an ortho pixel's depth for its k*k fine pixels; 1: the bilinear depth */
  float max_step;       /* interpolate only across depth differences <= max_step metres (> 0, finite) */
} pcp_ortho_texture_params;
int pcp_ortho_texture(pcp_context *ctx, const pcp_ortho_texture_params *params, uint8_t *out_rgb, uint8_t *out_mask,
                      uint8_t *out_status, int16_t *out_view, uint8_t *out_count, int64_t out_counts[4]);
/* Host only, no context, no GPU: the surface points alone ("raster" and "point" above) from a map's frame, source image and
 * depth layer as pcp_ortho_fetch / pcp_ortho_host return them.  out_xyz 3 floats per fine pixel (0 where there is no surface),
 * out_ok 1 where a surface exists; both nullable.  The message is at pcp_last_error(NULL). */
int pcp_ortho_texture_points_host(const pcp_ortho_frame *frame, const pcp_ortho_texture_params *params, const int32_t *source,
                                  const float *depth, float *out_xyz, uint8_t *out_ok);

/* ---- keyframe colour balance (scripts/image_color_balance_autonomous.py, scripts/image_color_balance.py) */
/* CLAHE on a lightness channel and a gamma table, applied on the device to every keyframe as it is uploaded instead of being
 * run over the keyframe folder beforehand and written back as new JPEGs ("Image balance", IB1-IB9).  Opt-in:
 * off by default, nothing runs unless pcp_set_image_balance turns it on, PCP_ABI_VERSION is unchanged and a caller detects
 * support by the symbols.  pcp_image_balance's kernels are timed under PCP_K_MISC.
 *
 * Stated differences from the scripts: the lightness channel is V of the 8-bit BGR -> HSV conversion pcp_set_image_adjust
 * uses, not L of 8-bit Lab (apply_clahe, image_color_balance_autonomous.py:17-23 and image_color_balance.py:34-40: cvtColor
 * BGR2LAB, clahe.apply(l), merge, LAB2BGR), and the balanced pixels are never re-encoded as JPEG (cv2.imwrite,
 * image_color_balance_autonomous.py:110, image_color_balance.py:81).  Parity with OpenCV's pixels is unpinned. */
#define PCP_BALANCE_CLAHE 1 /* steps 1-3: V -> CLAHE -> back to BGR (apply_clahe, image_color_balance_autonomous.py:100) */
#define PCP_BALANCE_GAMMA 2 /* step 4: the table on B, G, R (adjust_gamma, image_color_balance_autonomous.py:25-28, :103) */
typedef struct pcp_balance_params {
  int32_t stages;           /* PCP_BALANCE_* bits; 0 = off */
  int32_t tiles_x, tiles_y; /* tileGridSize, each 1..16 */
  float clip_limit;         /* clipLimit; <= 0: no clipping */
  float gamma;              /* adjust_gamma's gamma, > 0; 1 = identity table */
} pcp_balance_params;
/* image_color_balance_autonomous.py:116-120 main(): clip 1.0, tiles 8 x 8, gamma 0.8, both stages (image_color_balance.py:74,77:
 * clip 3.0, gamma 1.1) */
void pcp_default_balance_params(pcp_balance_params *p);
/* Applies to images uploaded afterwards through pcp_upload_image[_async], pcp_upload_images_block and
 * pcp_upload_image_jpeg[_async], like pcp_set_image_adjust: the texels of a keyframe uploaded with balance on are, bit for
 * bit, those of the same upload with balance off from the image pcp_image_balance_host produces; pcp_set_image_adjust's
 * round trip, when enabled, comes after the balance, and the mask byte is untouched.  NULL or stages == 0: off.  Tiles
 * outside 1..16, gamma <= 0, a non-finite value or unknown stage bits: PCP_ERR_INVALID and the setting is unchanged.  With
 * CLAHE on, an upload to a camera whose image the tile grid cannot be reflected over (see below) returns PCP_ERR_RANGE. */
int pcp_set_image_balance(pcp_context *ctx, const pcp_balance_params *params);
/* Host only, no context, no GPU: w x h BGR8 rows in, w x h tightly packed BGR8 out (out_bgr nullable), by the arithmetic the
 * kernels use (csrc/pcp_image_balance.hpp).  out_hist (nullable): the raw per-tile V histograms before clipping,
 * tiles_y * tiles_x * 256; out_lut (nullable): the per-tile tables, tiles_y * tiles_x * 256 bytes; both written only with
 * PCP_BALANCE_CLAHE.  When w % tiles_x or h % tiles_y is not 0 the image counts as extended to the right by
 * tiles_x - w % tiles_x columns and at the bottom by tiles_y - h % tiles_y rows (a side that divides evenly by a whole
 * tiles_x / tiles_y, as OpenCV does), read through BORDER_REFLECT_101; an extension >= w or >= h: PCP_ERR_RANGE.  Bad
 * parameters (as above), w or h < 1, a NULL image or a row stride < 3 w: PCP_ERR_INVALID.  Message at pcp_last_error(NULL). */
int pcp_image_balance_host(const pcp_balance_params *params, int32_t w, int32_t h, const uint8_t *bgr, int64_t row_stride_bytes,
                           uint8_t *out_bgr, uint32_t *out_hist, uint8_t *out_lut);
/* The same on the device for an arbitrary image, independent of the camera and of pcp_set_image_balance / _adjust: the pack,
 * histogram, table and apply kernels the upload path runs, on scratch texels, and an unpack.  Synchronous; it waits for
 * uploads in flight.  Same arguments, outputs and returns as the host form. */
int pcp_image_balance(pcp_context *ctx, const pcp_balance_params *params, int32_t w, int32_t h, const uint8_t *bgr,
                      int64_t row_stride_bytes, uint8_t *out_bgr, uint32_t *out_hist, uint8_t *out_lut);
/* adjust_gamma (image_color_balance_autonomous.py:25-28): table[i] = (uint8)(pow(i / 255.0, 1.0 / gamma) * 255.0), fp64, truncated.  gamma <= 0 or not
 * finite: PCP_ERR_INVALID. */
int pcp_gamma_table_host(float gamma, uint8_t out[256]);

/* ---- geometry maps (scripts/genNormAndDistanceMask.py: class Crack, generate_norm_masks :200-231, generate_distance_masks :233-266) */
/* A normal per point of the uploaded map and, per keyframe, the images the crack measurement reads: range, camera position,
 * camera normal and the index of the point behind every pixel ("Geometry maps", GN1-GN7 and GM1-GM5).  Opt-in:
 * nothing runs unless one of these is called, PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.
 * Kernels are timed under PCP_K_MISC.
 *
 * pcp_estimate_normals: once per uploaded cloud, in the world frame, over ALL neighbours within `radius`
 * (0.005 <= radius <= 1, else PCP_ERR_INVALID).  The finite points are queries and candidates; j is a neighbour of i iff
 * fl32((dx*dx + dy*dy) + dz*dz) <= t with d = fl32(p_j - p_i) and t the largest float with (double)t <= (double)radius^2; a
 * point is its own neighbour.  Each accepted d is quantised to q = rint(d * 2^20) and the moments about the query -- n,
 * S1[a] = sum q_a, S2[ab] = sum q_a q_b -- are exact 64-bit sums, so the result does not depend on the order of the
 * neighbours or of the input.  C_ab = (double)S2_ab - ((double)S1_a * (double)S1_b) / (double)n; the normal is the
 * eigenvector of C's smallest eigenvalue ev (pcl::eigen33's closed form), curvature = ev / trace(C) (0 when the trace is
 * <= 0).  The SIGN of the world normal is unspecified.  A point is valid iff it is finite, n >= 3 and the three components
 * are finite; an invalid point has normal (0, 0, 0) and curvature 0, its neighbour count is reported either way (0 for a
 * non-finite point).  A point with 2^22 neighbours or more: PCP_ERR_RANGE.  *out_valid (nullable) = valid points.
 * out_moments (nullable, host): 10 int64 per point in input order: n S1x S1y S1z S2xx xy xz yy yz zz.
 * The result stays on the device (20 B per point) until the next pcp_upload_cloud* drops it.  Like every call that builds
 * the search grid, it invalidates an open pcp_mls_stream / pcp_cloud_smooth_stream and a pcp_sor_partial.
 * pcp_normals_fetch: the result in input order, every output nullable: out_normal 3 floats per point, out_curvature and
 * out_neighbours one each.  Without an estimate on this cloud: PCP_ERR_STATE.
 * pcp_normals_moments_host: host only, no context, no GPU: the moments of n <= 65536 points (xyz interleaved) by brute force
 * over the pairs with the arithmetic the kernel uses (csrc/pcp_normals.hpp).  The message is at pcp_last_error(NULL).
 *
 * pcp_frame_geometry: images of image_width x image_height, row-major, every output nullable (host):
 *   contributors  exactly the points pcp_frame_visible lists for the keyframe (kept by the configured cull, any cull_mode and
 *                 depth source, and with a colour pixel); the pixel is pcp_project_frame's out_pixel;
 *   winner        the contributor with the smallest fp32 range (pcp_project_frame's out_range), ties to the lowest input index;
 *   out_index     the winner's input index, -1 for an empty pixel;  out_range its range;  out_xyz_cam 3 floats per pixel, the
 *                 camera coordinates pcp_frame_visible returns;  out_normal_cam 3 floats per pixel: R * n_world (R the rotation
 *                 of the keyframe's fp32 w2c, fp32, x*c0 + (y*c1 + z*c2)), negated when fl32((nx*x + ny*y) + nz*z) > 0 so
 *                 that it faces the camera; an invalid normal stays (0, 0, 0).  Empty pixels hold 0 in the float images.
 *   *out_pixels   occupied pixels.
 * out_normal_cam without pcp_estimate_normals on this cloud: PCP_ERR_STATE.  The images' device buffers (40 B per pixel)
 * are allocated on first use and freed by pcp_destroy. */
int pcp_estimate_normals(pcp_context *ctx, float radius, int64_t *out_valid, int64_t *out_moments);
int pcp_normals_fetch(pcp_context *ctx, float *out_normal, float *out_curvature, int32_t *out_neighbours);
int pcp_normals_moments_host(float radius, int64_t n, const float *xyz, int64_t *out_moments);
int pcp_frame_geometry(pcp_context *ctx, int32_t frame, int32_t *out_index, float *out_range, float *out_xyz_cam,
                       float *out_normal_cam, int64_t *out_pixels);

/* ---- map comparison (no counterpart in the reference; the method is Lague et al.'s M3C2) ---------------------------------- */
/* Per point of the uploaded map (the current survey), the signed distance along its normal to an earlier survey of the same
 * structure (the base), with a level of detection from the two epochs' scatter ("Map comparison", MC1-MC9).  Opt-in:
 * nothing runs unless one of these is called, PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.
 * Kernels are timed under PCP_K_MISC.  Whole-map contexts only; no streamed form.
 *
 * pcp_compare_set_base: the base, n_base host rows of stride_bytes (a multiple of 4, >= 12) with xyz first; copied to the
 * device, non-finite rows left out.  It replaces an earlier base (and ends its result) and stays across pcp_upload_cloud*
 * until pcp_compare_end or pcp_destroy.  n_base == 0 is allowed.  n + n_base <= 2^31 - 64.
 * pcp_compare: core points are the map points with three finite coordinates and a valid normal (three finite components,
 * each |n_a| <= 1, not all zero) -- `normals` (host, 3 floats per point, input order) or, when NULL, the live estimate of
 * pcp_estimate_normals (without one: PCP_ERR_STATE).  The normal is oriented by orient_mode (0: kept; 1: towards the point
 * orient; 2: along the vector orient; flipped iff fl32((nx*vx + ny*vy) + nz*vz) < 0 with v = fl32(orient - p) or orient),
 * then N_a = rint(n_a * 2^11), N2 = N.N (N2 == 0: not a core point).  In each epoch (A the map, B the base) point j is a
 * candidate of core point i iff, with d = fl32(p_j - p_i), q = rint(d * 2^20), h = q.N, Q2 = q.q:
 *   fl32((dx*dx + dy*dy) + dz*dz) <= t   (t the largest float with (double)t <= (double)s^2,
 *                                         s = nextafterf(fl32(sqrt((double)rc^2 + (double)L^2)), +inf)),
 *   h*h <= L2*N2 and Q2*N2 - h*h <= rc2*N2   (rc2 = floor((rc * 2^20)^2), L2 = floor((L * 2^20)^2), int64).
 * 0.005 <= cyl_radius, 0.005 <= cyl_half_length, s <= 0.5, reg_error finite and >= 0, min_points >= 2, orient_mode 0..2:
 * else PCP_ERR_INVALID.  Per epoch n, S1 = sum h, S2a = sum (h*h mod 2^32), S2b = sum (h*h div 2^32) are exact int64 sums
 * (an epoch with 2^22 candidates or more at one point: PCP_ERR_RANGE).  In fp64, every operation rounded on its own:
 *   S2 = (double)S2a + 4294967296.0 * (double)S2b;  scale = sqrt((double)N2) * 1048576.0;
 *   distance = ((double)S1A / nA - (double)S1B / nB) / scale;  var = (S2 - (S1 * S1) / n) / (n - 1.0) (below 0: 0);
 *   lod = 1.96 * sqrt(varA / nA + varB / nB) / scale + (double)reg_error.
 * Positive: the map's surface lies nearer the oriented side than the base's (deposit, bulge); negative: loss, spall.
 * status: 0 not a core point; 1 nB < min_points (no counterpart; distance and lod 0); 2 nA < min_points; 3 measured,
 * |distance| <= lod (compared in fp64); 4 significant, positive; 5 significant, negative.  Tests in that order.
 * out_stats (nullable): core points (status != 0), measured (3..5), significant positive, significant negative, no
 * counterpart, too few own points, most candidates of one epoch at one point, 0.
 * The result stays on the device (85 B per point) until the next pcp_upload_cloud* drops it.  Like every call that builds the
 * search grid, pcp_compare invalidates an open pcp_mls_stream / pcp_cloud_smooth_stream and a pcp_sor_partial; it touches
 * nothing else.  Without a cloud or a base: PCP_ERR_STATE.  Base points without a counterpart on the map are found by a second
 * run with the roles swapped (not built).
 * pcp_compare_fetch: the result in input order, every output nullable: distance, lod (float), status (uint8), 8 int64 sums
 * (nA S1A S2aA S2bA nB S1B S2aB S2bB) and the 3 int32 of N per point.  Without a result: PCP_ERR_STATE.
 * pcp_compare_host: host only, no context, no GPU: the same by brute force over the pairs with the arithmetic the kernel
 * uses (csrc/pcp_compare.hpp); n, n_base <= 65536, xyz / normals / base_xyz interleaved.  The message is at
 * pcp_last_error(NULL).
 * pcp_compare_end: drops the base and the result. */
typedef struct pcp_compare_params {
  float cyl_radius, cyl_half_length, reg_error;
  int32_t min_points, orient_mode;
  float orient[3];
} pcp_compare_params;
void pcp_default_compare_params(pcp_compare_params *p); /* 0.03, 0.05, 0, 5, mode 0 */
int pcp_compare_set_base(pcp_context *ctx, const void *points, int64_t n_base, int64_t stride_bytes);
int pcp_compare(pcp_context *ctx, const pcp_compare_params *p, const float *normals, int64_t out_stats[8]);
int pcp_compare_fetch(pcp_context *ctx, float *out_distance, float *out_lod, uint8_t *out_status, int64_t *out_sums8,
                      int32_t *out_direction3);
int pcp_compare_host(const pcp_compare_params *p, int64_t n, const float *xyz, const float *normals, int64_t n_base,
                     const float *base_xyz, float *out_distance, float *out_lod, uint8_t *out_status, int64_t *out_sums8,
                     int32_t *out_direction3, int64_t out_stats[8]);
int pcp_compare_end(pcp_context *ctx);

/* ---- map registration (no counterpart in the reference; the method is point-to-plane ICP, Chen & Medioni 1992) ------------- */
/* Fine registration of the base of the map comparison onto the uploaded map, before pcp_compare measures the change
 * ("Map registration", RG1-RG9).  Opt-in: nothing runs unless one of these is called, PCP_ABI_VERSION is unchanged
 * and a caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.  Whole-map contexts only.
 *
 * State: the context keeps the base's original rows and a rigid transform T, the identity after pcp_compare_set_base:
 * x' = R (x - c) + c + t with R from a unit quaternion (fp64), c the midpoint of the box of the base's finite rows,
 * (min + max) * 0.5 per axis in fp64, and ell half that box's diagonal (1 for a box without extent).  The rows pcp_compare
 * sees are fl32 of that, computed in fp64 from the ORIGINAL rows in a fixed order (csrc/pcp_register.hpp, apply); with T the
 * identity they are the original bytes.  A call that changes T drops a compare result.
 * pcp_compare_register_sums: one evaluation at the current T.  Queries: the finite base rows whose row index is a multiple
 * of sample_stride.  The partner of row b' is the finite map point p_j with the least fl32((dx*dx + dy*dy) + dz*dz), d =
 * fl32(p_j - b'), ties to the lowest index, if that is <= t (t the largest float with (double)t <= (double)match_radius^2);
 * no partner, or a partner whose normal is invalid (as in pcp_compare), is no pair.  `normals` as in pcp_compare.  With N_a
 * = rint(n_a * 2^11), q = rint(d * 2^20), h = q.N, N2 = N.N, u_a = rint((b'_a - c_a) * 2^8) and g = (u x N, N), the pair
 * counts iff h*h <= tau2 * N2, tau2 = floor((max_plane_distance * 2^20)^2).  Its thirty terms -- g_a g_b (a <= b, row by
 * row), g_a h, h h, N2, 1 -- are summed over all pairs, term k as out_sums60[2 k] = sum of (term mod 2^32) and
 * out_sums60[2 k + 1] = sum of (term div 2^32, arithmetic).  0.005 <= match_radius <= 0.5, 0 < max_plane_distance <=
 * match_radius, sample_stride >= 1, 1 <= max_iterations <= 1000, min_pairs >= 1, 0 <= tolerance <= 1, 0 < cond_tol < 1: else
 * PCP_ERR_INVALID.  A base whose current box reaches beyond |u_a| = 2^18 (1024 m from c): PCP_ERR_RANGE.  Without a cloud,
 * a base or normals: PCP_ERR_STATE.  Like every call that builds the search grid it invalidates an open pcp_mls_stream /
 * pcp_cloud_smooth_stream and a pcp_sor_partial; it touches nothing else.
 * pcp_register_solve_host: host only.  The update from the sums in fp64, every operation rounded on its own: the 6 x 6
 * normal equations with the rotation columns scaled by 1 / (2^19 ell) and the others by 2^-11, cyclic Jacobi (12 sweeps,
 * pairs p < q row by row, t = sign / (|theta| + sqrt(theta^2 + 1))), the solution in the span of the eigenvectors with
 * lambda_k > 0 and lambda_k >= cond_tol * lambda_max; *out_dof their number.  out_update7: omega (rad), dt (m), and rms =
 * sqrt(sum h^2 / sum N2) / 2^20 (m).  out_eigenvalues6 in the order of the diagonal.  Outputs nullable.
 * pcp_compare_register: the loop.  Per iteration: the sums at T; fewer than min_pairs pairs ends it with status 2 and T as
 * it was before that iteration; else the update is composed onto T (quaternion normalise(1, omega / 2), renormalised) and
 * the loop ends with status 0 when |omega| ell and |dt| are both below tolerance, or with status 1 after max_iterations.
 * out_T16: row-major 4 x 4.  out_log: max_iterations rows of 5 doubles (pairs, rms, dof, |omega| ell, |dt|), zeros after the
 * last.  out_status: the status, the rows written.  The rms of the last row is what a caller may pass as reg_error; nothing
 * applies it.  An error leaves T as it was.
 * pcp_compare_base_transform: T as a 4 x 4, the pivot, ell (each nullable).  pcp_compare_set_base_transform: a caller's rigid
 * 4 x 4 (last row 0 0 0 1, rotation orthonormal to 1e-9, det > 0: else PCP_ERR_INVALID); the identity restores the original
 * bytes.  Both need a base (PCP_ERR_STATE).
 * pcp_compare_register_host: host only, no context, no GPU: the same by brute force over the pairs with the arithmetic the
 * kernels use; n, n_base <= 65536, arrays interleaved.  T_in16 NULL: the identity.  run_loop 0: one evaluation at T_in
 * (out_sums60); else the loop from T_in (out_sums60: the last evaluation).  out_rows (nullable): the 3 n_base current rows
 * at the final T.  It also asserts the ranges of every pair in 128-bit arithmetic.  The message is at pcp_last_error(NULL). */
typedef struct pcp_register_params {
  float match_radius, max_plane_distance;
  int32_t sample_stride, max_iterations, min_pairs;
  double tolerance, cond_tol;
} pcp_register_params;
void pcp_default_register_params(pcp_register_params *p); /* 0.05, 0.02, 1, 20, 100, 1e-5, 6.2e-3 */
int pcp_compare_register_sums(pcp_context *ctx, const pcp_register_params *p, const float *normals, int64_t *out_sums60);
int pcp_register_solve_host(const int64_t *sums60, double ell, double cond_tol, double *out_update7, double *out_eigenvalues6,
                            int32_t *out_dof);
int pcp_compare_register(pcp_context *ctx, const pcp_register_params *p, const float *normals, double *out_T16, double *out_log,
                         int32_t *out_status);
int pcp_compare_base_transform(pcp_context *ctx, double *out_T16, double *out_pivot3, double *out_ell);
int pcp_compare_set_base_transform(pcp_context *ctx, const double *T16);
int pcp_compare_register_host(const pcp_register_params *p, int64_t n, const float *xyz, const float *normals, int64_t n_base,
                              const float *base_xyz, const double *T_in16, int32_t run_loop, int64_t *out_sums60, double *out_T16,
                              double *out_log, int32_t *out_status, float *out_rows);

/* ---- coarse registration (no counterpart in the reference; spin images, Johnson & Hebert 1999; Horn 1987) ------------------- */
/* Coarse registration of the base of the map comparison onto the uploaded map from an arbitrary pose, good enough for
 * pcp_compare_register to finish ("Coarse registration", CG1-CG9).  Opt-in: nothing runs unless one of these is
 * called, PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.
 * Whole-map contexts only.  side 0 is the uploaded map, side 1 the base's ORIGINAL rows (whatever its transform is).
 *
 * Keypoints (CG1): the rows whose index is a multiple of the side's stride, with three finite coordinates and a valid normal
 * (as in pcp_compare_register).  A keypoint's slot is row / stride; a side has ceil(rows / stride) slots, at most 2^18 (else
 * PCP_ERR_RANGE: raise the stride).  Map normals: `normals` (3 floats per point) or, NULL, the live estimate of
 * pcp_estimate_normals.  Base normals: `base_normals` (3 floats per row handed to pcp_compare_set_base) or, NULL, estimated
 * on the device at normal_radius over the original rows by the normals stage's own code; the map's live estimate is not
 * touched, and pcp_compare_base_normals_fetch returns the estimate (3 floats per row; PCP_ERR_STATE without one).
 * Descriptor (CG2): with N = rint(n * 2^11), N2 = N.N, and for every finite point of the SAME side within support_radius
 * (fl32 d2 <= t as in pcp_estimate_normals, the keypoint included) q = rint(d * 2^20), h = q.N, W = q.q * N2 - h*h: radial bin
 * = the largest k <= 7 with e_k^2 * N2 <= W, height bin likewise with h*h, e_k = floor(k * E / 8), E = rint(support_radius *
 * 2^20).  n_i = the number of neighbours; the descriptor is valid iff n_i >= min_neighbours and (n_i - those of height bin 0)
 * * 1000 >= min_offplane_permille * n_i; D[radial * 8 + height] = floor(count * 65535 / n_i).
 * pcp_coarse_descriptors: one side; out_counts3 = slots, keypoints, valid descriptors.  _fetch: per slot 64 uint16, n_i, the
 * state (0 no keypoint, 1 keypoint without a valid descriptor, 2 valid) and the keypoint's coordinates (each nullable).
 * The map's descriptors live until the next upload or pcp_estimate_normals, the base's until the next pcp_compare_set_base.
 * Matching (CG3), pcp_coarse_match: needs both sides' descriptors.  Ordinals count the valid descriptors of a side in
 * ascending row.  Key = (L1 << 32 | ordinal), L1 the exact sum of |D_a - D_b|; per valid keypoint the least and the second
 * least key over the other side.  (b, m) corresponds iff m is b's best, L1_best * 256 <= ratio_q8 * L1_second (no second: it
 * passes) and, with mutual, b is m's best; more than 2^18: PCP_ERR_RANGE.  _fetch: out_pairs (2 per correspondence: base
 * ordinal, map ordinal), out_base_keys / out_map_keys (2 uint64 per valid keypoint; ~0 = none), each nullable.
 * Scoring (CG5), pcp_coarse_score: n_frames frames of 15 doubles (R row-major, pivot c, t: x' = R (x - c) + c + t in
 * csrc/pcp_register.hpp's fixed fp64 sequence) over the live correspondences: b' = fl32(x'), d = fl32(m - b'), an inlier iff
 * every |d_a| <= 1 and q.q <= floor((inlier_distance * 2^20)^2).  out_counts: one per frame; out_flags (nullable): one byte
 * per frame and correspondence.
 * pcp_compare_register_coarse: the whole stage.  Hypothesis h < hypotheses draws three correspondences (splitmix64's
 * finaliser over seed + 0x9E3779B97F4A7C15 * (3 h + slot + 1), the high 32 bits times C, shifted right by 32) and is refused
 * when an ordinal repeats (1), a map side is shorter than min_side (2), a side differs between the clouds by more than
 * side_tolerance (3) or either triangle's smallest angle is below min_angle_deg (4: |s12 x s13|^2 < sin^2(min_angle_deg) times
 * the squared product of its two longest sides); else its frame
 * takes the base triangle's orthonormal frame and centroid onto the map's.  The winner has the most inliers (ties: lowest h);
 * fewer than min_inliers: status 2 and the base's transform stays.  Else Horn's quaternion solution over the winner's inliers
 * (exact integer sums of 2^-16 m quanta about the two boxes' midpoints, 4 x 4 cyclic Jacobi, 12 sweeps) is scored once and
 * kept iff it has at least as many inliers, and the kept frame is set exactly as pcp_compare_set_base_transform would
 * (a compare result is dropped).  out_report16: keypoints map, base; valid descriptors map, base; correspondences; hypotheses
 * scored, refused; inliers of the winner, of the best hypothesis rotated more than 10 degrees from it, of the refit, kept;
 * status (0 found, 2 too few inliers); the winner's h and its three ordinals (-1 without).  out_T16: the base's transform
 * after the call.  out_inliers (nullable, 2^18 bytes suffice): one byte per correspondence under the kept frame.
 * Bounds (else PCP_ERR_INVALID; NaN fails every test): 0.02 <= support_radius <= 0.25, 0.005 <= normal_radius <= 1, 0.005 <=
 * inlier_distance <= 0.5, 0 < min_side, 0 <= side_tolerance, 0 < min_angle_deg <= 60, strides >= 1, min_neighbours >= 1, 0 <=
 * min_offplane_permille <= 1000, 0 <= ratio_q8 <= 256, mutual 0 or 1, 1 <= hypotheses <= 65536, min_inliers >= 3.  Without a
 * cloud, a base, map normals, or the stage before: PCP_ERR_STATE.  Like every call that builds the search grid the
 * descriptor calls invalidate an open pcp_mls_stream / pcp_cloud_smooth_stream and a pcp_sor_partial.
 * The _host forms: host only, no context, no GPU, the same by brute force with the arithmetic the kernels use; n, n_base <=
 * 65536, arrays interleaved, base_normals required.  They also assert CG2's ranges per pair in 128-bit arithmetic.
 * pcp_coarse_hypothesis_host: hypothesis h over C correspondences (cb, cm: 3 floats each) about pivot3: the refusal code,
 * the three ordinals, the frame.  pcp_coarse_refit_host: CG6's refit over the flagged correspondences.  The message is at
 * pcp_last_error(NULL). */
typedef struct pcp_coarse_params {
  float support_radius, normal_radius, inlier_distance, min_side, side_tolerance, min_angle_deg;
  int32_t map_stride, base_stride, min_neighbours, min_offplane_permille, ratio_q8, mutual, hypotheses, min_inliers;
  uint64_t seed;
} pcp_coarse_params;
void pcp_default_coarse_params(pcp_coarse_params *p); /* 0.2, 0.1, 0.05, 0.3, 0.05, 15; 4, 4, 20, 100, 230, 1, 4096, 10; 1 */
int pcp_coarse_descriptors(pcp_context *ctx, const pcp_coarse_params *p, int32_t side, const float *normals, int64_t *out_counts3);
int pcp_coarse_descriptors_fetch(pcp_context *ctx, int32_t side, uint16_t *out_desc64, uint32_t *out_total, uint8_t *out_state,
                                 float *out_xyz);
int pcp_compare_base_normals_fetch(pcp_context *ctx, float *out_normals);
int pcp_coarse_match(pcp_context *ctx, const pcp_coarse_params *p, int64_t *out_count);
int pcp_coarse_match_fetch(pcp_context *ctx, int32_t *out_pairs, uint64_t *out_base_keys, uint64_t *out_map_keys);
int pcp_coarse_score(pcp_context *ctx, const pcp_coarse_params *p, int64_t n_frames, const double *frames15, int64_t *out_counts,
                     uint8_t *out_flags);
int pcp_compare_register_coarse(pcp_context *ctx, const pcp_coarse_params *p, const float *normals, const float *base_normals,
                                int64_t *out_report16, double *out_T16, uint8_t *out_inliers);
int pcp_coarse_descriptors_host(const pcp_coarse_params *p, int32_t side, int64_t n, const float *xyz, const float *normals,
                                uint16_t *out_desc64, uint32_t *out_total, uint8_t *out_state, int64_t *out_counts3);
int pcp_coarse_match_host(const pcp_coarse_params *p, int64_t k_base, const uint16_t *base_desc64, int64_t k_map,
                          const uint16_t *map_desc64, int32_t *out_pairs, int64_t *out_count, uint64_t *out_base_keys,
                          uint64_t *out_map_keys);
int pcp_coarse_hypothesis_host(const pcp_coarse_params *p, int64_t c, const float *cb, const float *cm, const double *pivot3, int32_t h,
                               int32_t *out_code, int32_t *out_triple3, double *out_frame15);
int pcp_coarse_score_host(const pcp_coarse_params *p, int64_t n_frames, const double *frames15, int64_t c, const float *cb,
                          const float *cm, int64_t *out_counts, uint8_t *out_flags);
int pcp_coarse_refit_host(int64_t c, const float *cb, const float *cm, const uint8_t *flags, const double *pivot_base3,
                          const double *pivot_map3, double *out_frame15);
int pcp_compare_register_coarse_host(const pcp_coarse_params *p, int64_t n, const float *xyz, const float *normals, int64_t n_base,
                                     const float *base_xyz, const float *base_normals, int64_t *out_report16, double *out_T16,
                                     uint8_t *out_inliers);

/* ---- mask distance maps (scripts/genNormAndDistanceMask.py: class Crack, preprocess :150-198, cv2.threshold :167, */
/* ---- scipy.ndimage.distance_transform_edt :9,168) ------------------------------------------------------------------ */
/* Per keyframe, the exact Euclidean distance transform of its mask and the nearest background pixel of every pixel (DESIGN.md,
 * "Mask distance maps", MD1-MD6).  Opt-in: nothing runs unless one of these is called, PCP_ABI_VERSION is unchanged and a
 * caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.
 *
 * Images of image_width x image_height of the context's camera, row-major, linear index y * W + x.  The mask byte m of a
 * pixel is the top byte of the keyframe's texel (pcp_upload_mask; what pcp_download_image returns as out_mask).
 *   threshold    0..255 (the script passes 0), else PCP_ERR_INVALID; a pixel is FOREGROUND iff m > threshold, else BACKGROUND;
 *   out_d2       uint32 per pixel: the minimum over the background pixels b of (bx - px)^2 + (by - py)^2, the exact integer, 0
 *                on a background pixel; sqrt((double)d2) is bit for bit what scipy.ndimage.distance_transform_edt(m > threshold)
 *                returns;
 *   out_nearest  int32 per pixel: the linear index of a background pixel at that distance -- of several the LOWEST index, i.e.
 *                the pixel that minimises the 64-bit key (d2 << 32) | index; a background pixel is its own nearest;
 *   a mask with NO background pixel gives d2 = 0xFFFFFFFF and nearest = -1 everywhere (scipy's result is then meaningless).
 * Both outputs are host pointers and nullable.  W or H above 16384: PCP_ERR_RANGE (keeps d2 below 2^30 and a row's working
 * set, 4 B per pixel, inside 64 KB of LDS).  A keyframe outside 0..n_frames-1 (or a negative count): PCP_ERR_RANGE.  A
 * keyframe without an uploaded mask, no camera or no keyframes: PCP_ERR_STATE.  No cloud is needed.
 * pcp_mask_edt_frames: keyframes first_frame .. first_frame + count - 1 in one call, `count` images back to back in each
 * output; a few launches for all of them (chunks of 2^26 pixels), not a few per keyframe.  count 0 does nothing.
 * Each call waits for the pending image uploads of its keyframes (the mask shares its word with the colour), is synchronous,
 * and invalidates nothing: the texels, the colour state, the depth maps and every other result stay as they are.  Device
 * buffers (12 B per pixel of one chunk, plus one bit per pixel) are allocated on first use and freed by pcp_destroy.
 * pcp_mask_edt_host: host only, no context, no GPU: the same results for a mask of `width` x `height` bytes with rows
 * row_stride_bytes apart (>= width), by the same arithmetic (csrc/pcp_mask_edt.hpp).  A NULL mask, an empty image or a bad
 * stride or threshold: PCP_ERR_INVALID; a side above 16384: PCP_ERR_RANGE.  The message is at pcp_last_error(NULL). */
int pcp_mask_edt(pcp_context *ctx, int32_t frame, int32_t threshold, uint32_t *out_d2, int32_t *out_nearest);
int pcp_mask_edt_frames(pcp_context *ctx, int32_t first_frame, int32_t count, int32_t threshold, uint32_t *out_d2,
                        int32_t *out_nearest);
int pcp_mask_edt_host(int32_t width, int32_t height, const uint8_t *gray, int64_t row_stride_bytes, int32_t threshold,
                      uint32_t *out_d2, int32_t *out_nearest);

/* ---- crack width maps (scripts/genNormAndDistanceMask.py: class Crack, compute_skeleton_edge_pts :396-478, ------------ */
/* ---- find_edges_by_direction / trace_edge :706-762, find_local_plane :601-636, search_3d_edge_points :564-599) -------- */
/* Per keyframe and per foreground pixel of its mask (a SITE): the two edge points along the exact EDT direction, the plane
 * of the position image's window around the pixel, and the 3-D distance between the intersections of the two edge rays with
 * that plane ("Crack width maps", CW1-CW9).  Opt-in: nothing runs unless one of these is called, PCP_ABI_VERSION
 * is unchanged and a caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.
 *
 * Images of image_width x image_height of the context's camera, row-major, linear index y * W + x.
 *   threshold        0..255: a pixel is foreground iff its mask byte exceeds it (as pcp_mask_edt);
 *   plane_radius_px  1..181 (the script uses 150): the plane's window is rows [max(0, y-R), min(H, y+R)), columns likewise;
 *   out_flags    one byte per pixel: bit 0 SITE, 1 CENTRE (d2 >= d2 of every 8-neighbour inside the image), 2 NEAR and 3 FAR
 *                (the trace towards / away from the nearest background pixel met a background pixel), 4 PLANE (3 members or
 *                more and a finite normal), 5 RAYS (both edge rays good), 6 WIDTH (= NEAR & FAR & PLANE & RAYS); 0 on
 *                background; a mask without a background pixel gives SITE only;
 *   out_edges    4 int32 per pixel: the near and the far edge point, each DOUBLED (E = last foreground pixel + first background
 *                pixel of the trace, x then y); -1 -1 for a side that is missing;
 *   out_w2d2     |E_far - E_near|^2 in half-pixel units, 0 unless NEAR and FAR;
 *   out_width    metres, fp32 of the fp64 norm; 0 without WIDTH;
 *   out_points   6 floats per pixel: X_near, X_far in camera coordinates; 0 without WIDTH;
 *   out_plane    4 floats per pixel: the unit normal facing the camera and -n.c; 0 without PLANE;
 *   out_moments  13 int64 per pixel: n, r[3], S1'[3], S2'[6] (xx xy xz yy yz zz) of the window's members, positions quantised to
 *                2^-16 m and recentred on the integer centroid r; exact; at every site, 0 on background;
 *   *out_sites, *out_widths   pixels with SITE / with WIDTH.
 * pcp_crack_width: every output is a host pointer and nullable.  Runs the keyframe's distance transform and geometry scatter
 * (no normals) on the device itself, then its own kernels; synchronous; waits for the keyframe's pending uploads like
 * pcp_mask_edt; invalidates nothing but the scratch images of pcp_mask_edt and pcp_frame_geometry.  No mask for the keyframe,
 * no cloud, no keyframes or no camera: PCP_ERR_STATE.  A keyframe outside 0..n_frames-1, a side above 16384 or W * H above
 * 2^26: PCP_ERR_RANGE.  A bad threshold or radius, or NULL params: PCP_ERR_INVALID.  Whole-map contexts only: an index shard
 * sees only its own points.  Device buffers (80 B per pixel for the tables plus the requested outputs) are allocated on first
 * use and freed by pcp_destroy.
 * pcp_crack_width_host: host only, no context, no GPU: flags bits 0-3, edges, w2d2 and moments by the same arithmetic
 * (csrc/pcp_crack_width.hpp) from a mask of `width` x `height` bytes with rows row_stride_bytes apart and the index and
 * xyz_cam images pcp_frame_geometry returns.  The message is at pcp_last_error(NULL). */
typedef struct pcp_crack_params {
  int32_t threshold;
  int32_t plane_radius_px;
} pcp_crack_params;
int pcp_crack_width(pcp_context *ctx, int32_t frame, const pcp_crack_params *params, uint8_t *out_flags, int32_t *out_edges,
                    uint32_t *out_w2d2, float *out_width, float *out_points, float *out_plane, int64_t *out_moments,
                    int64_t *out_sites, int64_t *out_widths);
int pcp_crack_width_host(int32_t width, int32_t height, const uint8_t *gray, int64_t row_stride_bytes, const int32_t *index_image,
                         const float *xyz_cam_image, const pcp_crack_params *params, uint8_t *out_flags, int32_t *out_edges,
                         uint32_t *out_w2d2, int64_t *out_moments);

/* ---- crack widths on the map (scripts/genNormAndDistanceMask.py: compute_skeleton_edge_pts :396-478, the result file :476-478) */
/* The widths pcp_crack_width measures per keyframe, brought back to the map points that see them, and the map's cracks as
 * connected components of the crack points ("Crack widths on the map", CF1-CF6 and CC1-CC6).  Opt-in: nothing
 * runs unless one of these is called, PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.  Kernels are
 * timed under PCP_K_MISC.  Whole-map contexts only: an index shard sees only its own points.
 *
 * Fusion.  pcp_crack_fuse_begin creates the accumulation for the uploaded cloud (40 B per point on the device): per point, in
 * input order, seen = added keyframes that list the point as a contributor (exactly pcp_frame_visible's list), views = those
 * whose pixel (pcp_project_frame's out_pixel) has WIDTH in pcp_crack_width's flags for the same keyframe and parameters,
 * centres = those whose pixel also has CENTRE, and over the credited keyframes sum_q, min_q (0xFFFFFFFF without one), max_q of
 * the quantum q = rint(width * 2^20), ties to even, 2^31 - 1 from 2048 m on, and the q of the keyframe with the smallest
 * (fp32 range, keyframe).  pcp_crack_fuse_add runs the keyframe's geometry scatter, distance transform and width kernels as
 * pcp_crack_width does (same checks and returns for the arguments they share; it invalidates what that call invalidates),
 * keeps the images on the device and adds the keyframe; *out_contributors / *out_credited (nullable) = listed / credited
 * points.  A keyframe is added once per accumulation: again is PCP_ERR_STATE and changes nothing, as does any failed add.
 * The final state does not depend on the order of the adds.  pcp_crack_fuse_fetch: all outputs nullable, n each, input order:
 *   width_mean = (float)(((double)sum_q / (double)views) * 2^-20), width_best = (float)((double)best_q * 2^-20), best_frame the
 *   keyframe of best_q; 0, 0 and -1 with views = 0.
 * pcp_crack_fuse_end releases it; pcp_upload_cloud*, pcp_set_camera and pcp_set_frames drop it.  _add, _fetch, _end,
 * pcp_crack_components and its fetch without a live accumulation: PCP_ERR_STATE.
 * pcp_crack_fuse_host: host only, no context, no GPU: one keyframe's add on caller-held state arrays of n points by the same
 * arithmetic (csrc/pcp_crack_fuse.hpp): m contributors (index into the state, pixel y * W + x, positive finite range) against
 * the width x height flag and width images.  A bad entry: PCP_ERR_INVALID and nothing changed.  Message at pcp_last_error(NULL).
 *
 * Cracks.  pcp_crack_components reads the live accumulation: point i is a crack point iff views[i] >= min_views
 * (1..4096) and its coordinates are finite; crack points i != j are linked iff fl32((dx*dx + dy*dy) + dz*dz) <= t with
 * d = fl32(p_j - p_i) and t the largest float with (double)t <= (double)radius^2 (pcp_estimate_normals' neighbour rule;
 * 0.005 <= radius <= 1); out_label (nullable, n, host) = the lowest input index of the point's connected component, -1 for a
 * point that is no crack point.  *out_crack_points / *out_components (nullable).  Bad parameters: PCP_ERR_INVALID.  Like every
 * call that builds the search grid it invalidates an open pcp_mls_stream / pcp_cloud_smooth_stream and a pcp_sor_partial.
 * pcp_crack_components_fetch: rows first .. first + max_rows - 1 of the table of that call, one row per crack, ascending by id
 * (= label): out_stats 5 int64 per row -- points, sum_w, min_w, max_w over the members' w = floor((2 sum_q + views) /
 * (2 views)), centre_points = members with centres > 0 -- and out_box 6 floats per row, the exact min x y z and max x y z of
 * the members' uploaded coordinates.  The table lives until the next _add, _end or drop of the accumulation.
 * pcp_crack_components_host: host only: the labels of n <= 65536 points (xyz interleaved) by brute force over the pairs. */
typedef struct pcp_crack_link_params {
  int32_t min_views;
  float radius;
} pcp_crack_link_params;
int pcp_crack_fuse_begin(pcp_context *ctx);
int pcp_crack_fuse_add(pcp_context *ctx, int32_t frame, const pcp_crack_params *params, int64_t *out_contributors,
                       int64_t *out_credited);
int pcp_crack_fuse_fetch(pcp_context *ctx, float *out_width_mean, float *out_width_best, int32_t *out_best_frame, uint32_t *out_views,
                         uint32_t *out_seen, uint32_t *out_centres, uint32_t *out_min_q, uint32_t *out_max_q, uint64_t *out_sum_q);
int pcp_crack_fuse_end(pcp_context *ctx);
int pcp_crack_fuse_host(int64_t n, uint32_t *seen, uint32_t *views, uint32_t *centres, uint32_t *min_q, uint32_t *max_q,
                        uint32_t *best_q, uint64_t *sum_q, uint64_t *best_key, int64_t m, const int32_t *index, const int32_t *pixel,
                        const float *range, int32_t frame, int32_t width, int32_t height, const uint8_t *flags, const float *width_image,
                        int64_t *out_credited);
int pcp_crack_components(pcp_context *ctx, const pcp_crack_link_params *p, int32_t *out_label, int64_t *out_crack_points,
                         int64_t *out_components);
int pcp_crack_components_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_stats, float *out_box,
                               int64_t *out_rows);
int pcp_crack_components_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, int32_t *out_label,
                              int64_t *out_components);

/* ---- crack lengths on the map (scripts/genNormAndDistanceMask.py orders a crack only by a 2-D skeleton per keyframe) ---------- */
/* The length of every crack of the map, its two end points, an ordered 3-D polyline through it and every crack point's arc
 * position ("Crack lengths on the map", CL1-CL9).  Opt-in: nothing runs unless one of these is called,
 * PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.  Whole-map
 * contexts only.
 *
 * pcp_crack_lengths reads the live accumulation under the crack points and links of pcp_crack_components for the same
 * parameters (same checks and returns; without a live accumulation PCP_ERR_STATE).  A link of squared distance d2 (the fp32
 * value the link rule compares) weighs w = max(1, isqrt(trunc((double)d2 * 2^40))) units of 2^-20 m; D_s(i) is the least sum
 * of weights from s to i.  Per crack: s0 = its id (the lowest input index), a = the lowest index among the maxima of D_s0,
 * b = the lowest index among the maxima of D_a, length_q = D_a(b) (the double sweep: exact on trees, a lower bound of the
 * diameter otherwise); the path runs from a to b, each point's predecessor the lowest index j linked to it with
 * D_a(j) + w = D_a(i).  out_pos (nullable, n, host) = D_a(i) for a crack point, 2^64 - 1 for every other point.
 * *out_cracks / *out_path_points (nullable) = rows of the table / entries of all paths.  The call runs the component stage
 * for its parameters: afterwards pcp_crack_components_fetch serves the table of these parameters, and the call invalidates
 * what pcp_crack_components invalidates.  PCP_ERR_DEVICE if a sweep does not settle within as many rounds as there are crack
 * points plus one (it cannot).
 * pcp_crack_lengths_fetch: rows first .. first + max_rows - 1 of that call's table, the rows and order of
 * pcp_crack_components_fetch: out_id, out_rows7 7 int64 per row -- end_a, end_b (input indices), length_q, hops,
 * path_sum_w, path_min_w, path_max_w over the fused w of the path's points -- and out_offsets (max_rows + 1 capacity; rows + 1
 * written): entry k = the first entry of row first + k in the path array, the last one the end of the last row fetched.
 * pcp_crack_paths_fetch: entries first_entry .. of the path array (input indices, a to b, hops + 1 per crack).  All outputs
 * nullable.  Table and paths live until the next _add, _end or drop of the accumulation.
 * pcp_crack_lengths_host: host only, no context, no GPU: the same results for n <= 65536 points (xyz interleaved) by brute
 * force over the pairs and a binary-heap Dijkstra; sum_q (nullable: every w = 0) and views give the fused w.  out_pos n,
 * out_id n, out_rows7 7 n, out_offsets n + 1, out_path n entries of capacity (all nullable). */
int pcp_crack_lengths(pcp_context *ctx, const pcp_crack_link_params *p, uint64_t *out_pos, int64_t *out_cracks, int64_t *out_path_points);
int pcp_crack_lengths_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows7, int64_t *out_offsets,
                            int64_t *out_rows);
int pcp_crack_paths_fetch(pcp_context *ctx, int64_t first_entry, int64_t max_entries, int32_t *out_index, int64_t *out_entries);
int pcp_crack_lengths_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, const uint64_t *sum_q,
                           uint64_t *out_pos, int32_t *out_id, int64_t *out_rows7, int64_t *out_offsets, int32_t *out_path,
                           int64_t *out_cracks, int64_t *out_path_points);

/* ---- crack skeletons on the map (scripts/genNormAndDistanceMask.py preprocess(): pcv.morphology.skeletonize, 2-D, per keyframe) -- */
/* The level-set diagram of every crack of the map: its branches, junctions and loops ("Crack skeletons on the
 * map", CS1-CS9).  Opt-in: nothing runs unless one of these is called, PCP_ABI_VERSION is unchanged and a caller detects
 * support by the symbols.  Kernels are timed under PCP_K_MISC.  Whole-map contexts only.
 *
 * pcp_crack_skeleton replaces the per-keyframe 2-D skeleton of the reference's script by one diagram per crack of the map.
 * It runs pcp_crack_lengths' stage for the parameters (same checks and returns; it leaves the component and length tables of
 * these parameters behind and invalidates what those calls invalidate), then cuts every crack into bands of its arc
 * position: step_q = trunc((double)step * 2^20), band(i) = pos[i] / step_q.  step_q must be at least the largest link weight
 * isqrt(trunc((double)t * 2^40)) of the radius and step at most 16, else PCP_ERR_INVALID; linked points then lie at most one
 * band apart.  A node is a connected component of the crack points under the links that join two points of one band, its id
 * the lowest input index among its points; out_node (nullable, n, host) = that id, -1 for a point that is no crack point.
 * An edge is an unordered pair of nodes with at least one link between their points.  *out_nodes / *out_edges (nullable) =
 * rows of the two tables.  PCP_ERR_RANGE if a crack point has a coordinate beyond 2^20 m (or the exact coordinate sums of
 * all crack points could pass 2^62); PCP_ERR_NOMEM if the edge set is still full after 12 doublings.
 * pcp_crack_skeleton_nodes_fetch: rows first .. of the node table, ascending by id: out_id, out_rows10 10 int64 per row --
 * crack_row (the row of pcp_crack_components_fetch), band, points, sum_w, min_w, max_w over the members' fused w, sum_qx,
 * sum_qy, sum_qz (sums of floor((double)x * 2^20) and likewise y, z: the centroid is (sum_q / points) * 2^-20), degree.
 * pcp_crack_skeleton_edges_fetch: out_rows3 3 int64 per row -- u (the row of the node in the lower band), v (the row of the
 * other; the bands differ by one), links (linked point pairs between them); unique, ascending by (u, v).
 * pcp_crack_skeleton_cracks_fetch: the rows and order of pcp_crack_components_fetch, out_rows6 6 int64 per row -- nodes,
 * edges, ends (degree 1), junctions (degree >= 3), loops = edges - nodes + 1, max_degree.  Replaces what the script's
 * compute_skeleton_edge_pts leaves to a hand count.  All outputs nullable; the tables live as long as pcp_crack_lengths' do.
 * pcp_crack_skeleton_host: host only, no context, no GPU: the same results for n <= 65536 points (xyz interleaved) by brute
 * force over the pairs, a sequential union-find and an ordered map; sum_q (nullable: every w = 0).  out_node n, out_id n,
 * out_rows10 10 n, out_rows6 6 n of capacity; out_rows3 takes at most edge_capacity rows, *out_edges is the whole count. */
int pcp_crack_skeleton(pcp_context *ctx, const pcp_crack_link_params *p, float step, int32_t *out_node, int64_t *out_nodes, int64_t *out_edges);
int pcp_crack_skeleton_nodes_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows10, int64_t *out_rows);
int pcp_crack_skeleton_edges_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int64_t *out_rows3, int64_t *out_rows);
int pcp_crack_skeleton_cracks_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int64_t *out_rows6, int64_t *out_rows);
int pcp_crack_skeleton_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, float step,
                            const uint64_t *sum_q, int32_t *out_node, int32_t *out_id, int64_t *out_rows10, int64_t edge_capacity,
                            int64_t *out_rows3, int64_t *out_rows6, int64_t *out_nodes, int64_t *out_edges, int64_t *out_cracks);

/* ---- crack directions on the map (scripts/evalSkeletonDirection.py only blurs one keyframe's 2-D skeleton and shows it) ------ */
/* Which way every crack of the map runs: a tangent per crack point and the sums per crack from which the host takes the
 * crack's axis ("Crack directions on the map", CD1-CD9).  Opt-in: nothing runs unless one of these is called,
 * PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.  The kernel is timed under PCP_K_MISC.  Whole-map
 * contexts only.
 *
 * pcp_crack_directions reads the live accumulation under the crack points and links of pcp_crack_components for the same
 * parameters (same checks and returns; without a live accumulation PCP_ERR_STATE).  It runs the component stage: afterwards
 * pcp_crack_components_fetch serves the table of these parameters, the tables of pcp_crack_lengths and pcp_crack_skeleton are
 * kept, and the call invalidates what pcp_crack_components invalidates.  Per crack point i, over its linked points j, the
 * offset d = fl32(p_j - p_i) is quantised to q = rint(d * 2^20) per axis (ties to even) and ten exact int64 moments are
 * summed: n (the links), S1 x y z, S2 xx xy xz yy yz zz -- a function of the set of links alone.  A point with 2^22 links or
 * more: PCP_ERR_RANGE.  With C the covariance of the moments (pcp_estimate_normals' three fp64 operations per entry) and l1
 * its largest eigenvalue, the tangent is valid iff n >= 2 and l1 > 0: the unit eigenvector of l1 taken in fp64, its component
 * of largest magnitude positive (ties: the lowest axis), stored as fp32; anisotropy = (float)(l1 / trace(C)), 1 on a line and
 * about 1/2 on a flat isotropic patch.  Otherwise tangent and anisotropy are zeros.  out_tangent 3 n, out_anisotropy n,
 * out_links n, out_moments 10 n: host, nullable, input order, zeros for a point that is no crack point.  *out_crack_points /
 * *out_cracks (nullable).
 * pcp_crack_directions_fetch: rows first .. first + max_rows - 1 of that call's table, the rows and order of
 * pcp_crack_components_fetch: out_id and out_rows20, 20 int64 per row -- for each of the ten moment words in the order above
 * the sum over the crack's members as (lo, hi): lo = the sum of (v & 0xffffffff), hi = the sum of (v >> 32) (arithmetic), the
 * value hi * 2^32 + lo.  Word 0 is the number of ordered links L; the three S1 sums are exactly zero (every link is counted
 * from both ends with opposite offsets).  The table lives until the next _add, _end or drop of the accumulation; later
 * pcp_crack_components / _lengths / _skeleton keep it.
 * pcp_crack_directions_host: host only, no context, no GPU: the same results for n <= 65536 points (xyz interleaved) by brute
 * force over the pairs; out_id n and out_rows20 20 n of capacity (all outputs nullable).
 * pcp_crack_axis_host: host only, fp64: out5 = L, the unit eigenvector of the largest eigenvalue of S2 / L under the sign rule
 * above, and its anisotropy, the words rebuilt as (double)hi * 2^32 + (double)lo.  L < 2 or a zero largest eigenvalue: axis
 * (0, 0, 0) and anisotropy 0.  A NULL argument: PCP_ERR_INVALID. */
int pcp_crack_directions(pcp_context *ctx, const pcp_crack_link_params *p, float *out_tangent, float *out_anisotropy, int32_t *out_links,
                         int64_t *out_moments, int64_t *out_crack_points, int64_t *out_cracks);
int pcp_crack_directions_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows20, int64_t *out_rows);
int pcp_crack_directions_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, float *out_tangent,
                              float *out_anisotropy, int32_t *out_links, int64_t *out_moments, int32_t *out_id, int64_t *out_rows20,
                              int64_t *out_cracks);
int pcp_crack_axis_host(const int64_t row20[20], double out5[5]);

/* ---- crack branches on the map (the reference's scripts never take a skeleton apart: an inspector's record goes arm by arm) -- */
/* The diagram of pcp_crack_skeleton cut at its junctions into branches, short spurs pruned, and one exact integer record per
 * branch ("Crack branches on the map", CB1-CB9).  Opt-in: nothing runs unless one of these is called,
 * PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.  Whole-map
 * contexts only.
 *
 * pcp_crack_branches (CB1-CB4, CB9) runs pcp_crack_skeleton's stage for the parameters and step (same checks and returns; it
 * leaves the component, length and skeleton tables of these parameters behind, keeps the table of pcp_crack_directions and
 * invalidates what pcp_crack_skeleton invalidates).  prune (metres): prune_q = trunc((double)prune * 2^20); 0 <= prune <= 1024
 * or PCP_ERR_INVALID (a NaN included); 0 prunes nothing.  In a set K of nodes with the edges between them a node of degree >= 3
 * is a junction; the branches are the connected components of the other nodes under the edges between two of them (paths or
 * cycles), a branch's attachments are its edges to junctions (0, 1 or 2), an edge between two junctions is a bridge.  The whole
 * diagram is decomposed once; a branch with exactly one attachment and nodes * step_q < prune_q that holds neither node[end_a]
 * nor node[end_b] of its crack (pcp_crack_lengths_fetch) is a spur.  One round: the final branches are the decomposition of the
 * nodes outside spurs, whatever their size; a junction left with two kept edges is an ordinary node.  A branch's id is the
 * lowest input index among its points.  out_branch (nullable, n, host) = that id, -1 for a point that is no crack point, -2
 * for a point of a kept junction, -3 for a point of a pruned node.  *out_branches / *out_pruned_branches (nullable).  A crack
 * point with 2^22 links or more inside its branch: PCP_ERR_RANGE.
 * pcp_crack_branches_fetch (CB5, CB6): rows first .. of the branch table, ascending by id: out_id; out_rows15 15 int64 per row
 * -- crack_row, nodes, edges_inside, attachments, junction_u, junction_v (the node rows of the junctions attached to, the lower
 * first; junction_v = -1 with one attachment, both -1 with none), points, sum_w, min_w, max_w (the fused w of the members),
 * pos_min, pos_max (pcp_crack_lengths' pos), sum_qx, sum_qy, sum_qz (as pcp_crack_skeleton_nodes_fetch); out_moments20 20 int64
 * per row -- the ten moment words of pcp_crack_directions_fetch as (lo, hi), summed over the ordered links whose two points
 * lie in this branch: pcp_crack_axis_host on such a row gives the branch's axis and anisotropy.  The S1 sums are exactly zero.
 * pcp_crack_branch_edges_fetch (CB7): one int32 per row of pcp_crack_skeleton_edges_fetch: the branch row of the edge (an edge
 * to a junction belongs to the branch of its other end), -1 for a bridge, -2 for an edge with a pruned end.
 * pcp_crack_branch_cracks_fetch (CB7): the rows and order of pcp_crack_components_fetch, out_rows7 7 int64 per row -- branches,
 * bridges, junctions_kept, ends_kept (kept nodes of degree 1 among the kept edges), pruned_branches, pruned_nodes,
 * pruned_points.  All outputs nullable; the tables live until the next pcp_crack_lengths, pcp_crack_skeleton, _add, _end or
 * drop of the accumulation; pcp_crack_components and pcp_crack_directions keep them.
 * pcp_crack_branches_host: host only, no context, no GPU: the same results for n <= 65536 points (xyz interleaved) by brute
 * force over the pairs; sum_q (nullable: every w = 0).  out_branch n, out_id n, out_rows15 15 n, out_moments20 20 n, out_rows7
 * 7 n of capacity; out_edge_branch takes at most edge_capacity rows, *out_edges is the whole count.
 * pcp_crack_branch_lengths_host (CB8): host only, fp64, the one expression every host layer uses: from the node and edge tables
 * of pcp_crack_skeleton and the edge_branch of pcp_crack_branch_edges_fetch, out_length_m[b] = the sum, in edge-row order and
 * one addition after the other, of the lengths of the edges with edge_branch == b (an edge's length is the distance of its two
 * nodes' centroids (sum_q / points) * 2^-20), out_kept_length_m[c] = the same over crack c's edges with edge_branch >= -1.  A
 * row that names a node, a branch or a crack that is not there, or a node without a point: PCP_ERR_INVALID. */
int pcp_crack_branches(pcp_context *ctx, const pcp_crack_link_params *p, float step, float prune, int32_t *out_branch, int64_t *out_branches,
                       int64_t *out_pruned_branches);
int pcp_crack_branches_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows15, int64_t *out_moments20,
                             int64_t *out_rows);
int pcp_crack_branch_edges_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_edge_branch, int64_t *out_rows);
int pcp_crack_branch_cracks_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int64_t *out_rows7, int64_t *out_rows);
int pcp_crack_branch_lengths_host(int64_t nodes, const int64_t *rows10, int64_t edges, const int64_t *rows3, const int32_t *edge_branch,
                                  int64_t branches, int64_t cracks, double *out_length_m, double *out_kept_length_m);
int pcp_crack_branches_host(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float radius, float step, float prune,
                            const uint64_t *sum_q, int32_t *out_branch, int32_t *out_id, int64_t *out_rows15, int64_t *out_moments20,
                            int64_t edge_capacity, int32_t *out_edge_branch, int64_t *out_rows7, int64_t *out_branches, int64_t *out_edges,
                            int64_t *out_cracks);

/* ---- planar facets of the map (the reference's scripts stop at per-keyframe pictures: no step partitions the map) ---------- */
/* The faces of the structure as connected components of the map points under a symmetric integer link, one row of exact
 * integers per face, its plane, and an orthographic map restricted to one face ("Planar facets", FA1-FA9).
 * Opt-in: nothing runs unless one of these is called, PCP_ABI_VERSION is unchanged and a caller detects support by the
 * symbols.  Kernels are timed under PCP_K_MISC.  Whole-map contexts only: an index shard sees only its own points.
 *
 * pcp_facets reads the uploaded cloud and the live estimate of pcp_estimate_normals (without one: PCP_ERR_STATE).  Point i is a
 * facet point iff its coordinates are finite, its stored normal is valid (not (0, 0, 0)) and its stored curvature <=
 * max_curvature (0 <= max_curvature <= 1).  N = rint(normal * 2^14) per component.  Facet points i != j are linked iff
 *   (a) fl32((dx*dx + dy*dy) + dz*dz) <= t with d = fl32(p_j - p_i) and t the largest float with (double)t <= link_radius^2
 *       (pcp_estimate_normals' neighbour rule; 0.005 <= link_radius <= 1),
 *   (b) |N_i . N_j| >= ceil(cos(angle_deg) * 2^28)   (0 < angle_deg <= 45; the normals' sign is unspecified), and
 *   (c) |N_i . q| and |N_j . q| <= floor(plane_tol * 2^34) with q = rint(d * 2^20)   (1e-4 <= plane_tol <= 0.1 metres),
 * all in exact 64-bit integers.  A facet is a connected component of the links with at least min_points members
 * (1..2^24); its id is the lowest input index among them.  out_label (nullable, n, host) = the id of the point's facet, -1 for
 * a point in none.  *out_facet_points / *out_components / *out_facets (nullable) = facet points, components of any size, facets.
 * Bad parameters: PCP_ERR_INVALID.  A facet with points * (D * 4096 + 1)^2 >= 2^62, D the largest extent of its box:
 * PCP_ERR_RANGE, the message names the facet.  Like every call that builds the search grid it invalidates an open
 * pcp_mls_stream / pcp_cloud_smooth_stream and a pcp_sor_partial.  Labels and table live until the next pcp_facets,
 * pcp_estimate_normals or pcp_upload_cloud*; a failed call leaves none.
 * pcp_facets_fetch: rows first .. first + max_rows - 1 of the table, one row per facet, ascending by id: out_id, out_rows10 10
 * int64 per row -- points, S1 x y z, S2 xx xy xz yy yz zz of Q = rint(fl32(p - p_root) * 2^12) over the members, p_root the
 * coordinates of point id -- and out_box 6 floats per row, the exact min x y z and max x y z of the members.  All outputs
 * nullable.  Without a table: PCP_ERR_STATE.  Negative first / max_rows: PCP_ERR_INVALID.
 * pcp_facets_host: host only, no context, no GPU: the same results for n <= 65536 points (xyz and normal interleaved) by brute
 * force over the pairs and a sequential union-find; out_label n, out_id n, out_rows10 10 n, out_box 6 n of capacity (all
 * nullable).  pcp_facet_plane_host: host only, fp64, the plane of one row: out_plane = centroid root + (S1 / points) * 2^-12,
 * the unit eigenvector of the smallest eigenvalue ev of S2 - S1 S1^T / points by pcl::eigen33's closed form, signed so that its
 * largest component is positive ((0, 0, 0) when the members span no plane), and rms = sqrt(max(ev, 0) / points) * 2^-12 metres.
 * points < 1 or a NULL argument: PCP_ERR_INVALID.  Messages of the two at pcp_last_error(NULL).
 * pcp_ortho_add_facet: pcp_ortho_add (same checks and returns) restricted to the rows whose facet label equals facet_id; the
 * colour and fused-label layers are kept.  Without live facets: PCP_ERR_STATE; facet_id outside 0 .. n - 1: PCP_ERR_RANGE. */
typedef struct pcp_facet_params {
  float link_radius, angle_deg, plane_tol, max_curvature;
  int32_t min_points;
} pcp_facet_params;
int pcp_facets(pcp_context *ctx, const pcp_facet_params *params, int32_t *out_label, int64_t *out_facet_points, int64_t *out_components,
               int64_t *out_facets);
int pcp_facets_fetch(pcp_context *ctx, int64_t first, int64_t max_rows, int32_t *out_id, int64_t *out_rows10, float *out_box,
                     int64_t *out_rows);
int pcp_facets_host(int64_t n, const float *xyz, const float *normal, const float *curvature, const pcp_facet_params *params,
                    int32_t *out_label, int32_t *out_id, int64_t *out_rows10, float *out_box, int64_t *out_facets);
int pcp_facet_plane_host(const float root[3], const int64_t row10[10], double out_plane[7]);
int pcp_ortho_add_facet(pcp_context *ctx, int32_t facet_id, int64_t index_base, int64_t *out_contributors);

/* ---- cylindrical facets (no counterpart in the reference: its pictures are per-keyframe perspective views) ----------------- */
/* A second kind of frame for the orthographic maps: a cylinder, unrolled along its arc ("Cylindrical facets",
 * CY1-CY9).  Image x runs along the arc R theta, image y along the axis, both at gsd metres per pixel; the depth layer is the
 * radial deviation side (rho - R) from the cylinder.  Opt-in: nothing runs unless one of these is called, PCP_ABI_VERSION is
 * unchanged and a caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.
 *   frame     c a point of the axis (row coordinate h = 0), a the unit axis (rows run along +a), e and b unit and perpendicular
 *             to a and to each other (theta = 0 along e, pi/2 along b), radius R in [0.05, 1000] metres, gsd in [1e-4, 1],
 *             width x height >= 1 x 1, d_min < d_max, side +1 (seen from inside, depth grows outward) or -1 (from outside).
 *             A non-finite value, a value outside these ranges, axes (e, b, a) that are not orthonormal with e x b = side a
 *             within 1e-3, or width gsd > 2 pi R + gsd: PCP_ERR_INVALID.  A raster past 16384 a side or 2^26 pixels:
 *             PCP_ERR_RANGE, the message names the gsd at which the same extent fits.
 *   point     d = fl32(p - c); s = d.e, t = d.b, h = d.a in fp32 (pcp_ortho's association); in fp64, every operation rounded on
 *             its own: rho = sqrt(s s + t t), theta in [0, 2 pi] by a fixed sequence of operations (no libm; CY3), arc = R theta;
 *             x = (float)(arc inv), y = fl32(h inv) with inv = fl32(1 / gsd); depth = (float)(side (rho - R)).  A row contributes
 *             iff its has bit is set, its coordinates are finite, rho > 0, 0 <= x < W, 0 <= y < H (in float) and
 *             d_min <= depth <= d_max; its pixel is (floor(x), floor(y)).  The map does not wrap across the seam theta = 0 | 2 pi.
 * pcp_ortho_begin_cyl starts the accumulator of pcp_ortho_begin under such a frame; either begin drops the live map of either
 * kind, a refused one leaves it.  pcp_ortho_add / _add_facet / _add_packed / _finish / _fetch / _stats / _end work on either kind,
 * with the same keys, merge, payload, fill and layers.  pcp_ortho_texture on a cylinder's map: PCP_ERR_STATE (orthophotos of
 * unrolled maps are not built by that call: pcp_ortho_texture_cyl, below).
 * pcp_ortho_cyl_host: pcp_ortho_host under a cylinder's frame, bit for bit what the device gives.
 * pcp_cyl_angle_host: theta of n pairs (s, t) of doubles by the same sequence (host only; (0, 0) gives a NaN).
 * pcp_cyl_fit_host: host only, fp64, closed form: the cylinder of the rows whose has byte is set (NULL: all), whose coordinates
 * are finite and whose normal (3 floats per row) is finite and not (0, 0, 0), and the frame that unrolls them so that every such
 * row contributes.  Axis: the eigenvector of the smallest eigenvalue of the normals' scatter, signed so that its largest component
 * is negative; centre and R: the algebraic circle through the rows projected along the axis; side +1 iff viewer (3 doubles,
 * nullable) lies within R of the axis; the seam in the longest empty stretch of 4096 angle bins (a ring whose longest stretch is
 * shorter than two pixels is closed: width = ceil(2 pi R / gsd)).  out_stats (nullable): rows used, rms, least and greatest of
 * rho - R, the occupied arc in radians, the three eigenvalues of the normals' scatter ascending.  Fewer than 16 rows, parallel
 * normals, R outside [0.05, 1000], a raster past the limits: PCP_ERR_RANGE.  Messages of the three at pcp_last_error(NULL). */
typedef struct pcp_cyl_frame {
  float c[3];        /* a point of the axis: where row coordinate h = 0 */
  float a[3];        /* unit axis: image y (rows) runs along +a */
  float e[3], b[3];  /* unit, perpendicular to a and to each other: theta = 0 along e, pi/2 along b */
  float radius;      /* R, metres */
  float gsd;
  int32_t width, height;
  float d_min, d_max;
  int32_t side;      /* +1: seen from inside (depth grows outward), -1: seen from outside */
} pcp_cyl_frame;
int pcp_ortho_begin_cyl(pcp_context *ctx, const pcp_cyl_frame *frame);
int pcp_ortho_cyl_host(const pcp_cyl_frame *frame, int64_t n, const float *xyz, const uint8_t *rgb, const uint8_t *label,
                       const uint8_t *has, int64_t index_base, int32_t fill_radius_px, uint32_t *out_index, float *out_depth,
                       uint8_t *out_rgb, uint8_t *out_label, uint8_t *out_status, int32_t *out_source, int64_t *out_contributors,
                       int64_t *out_occupied, int64_t *out_filled);
int pcp_cyl_angle_host(int64_t n, const double *s, const double *t, double *out_theta);
int pcp_cyl_fit_host(int64_t n, const float *xyz, const float *normal, const uint8_t *has, const double *viewer, float gsd,
                     pcp_cyl_frame *out, double out_stats[8]);
/* Orthophotos of unrolled maps ("Orthophotos of unrolled maps", CT1-CT8): pcp_ortho_texture for the finished map of
 * pcp_ortho_begin_cyl.  Same parameters, layers, counts, checks and check order as pcp_ortho_texture; a live planar map is
 * PCP_ERR_STATE (pcp_ortho_texture is its call).  Only the surface point differs, the inverse of "pixel" above in fp64:
 *   xf = (Xg + 0.5) / k, yf likewise; arc = xf / inv, hh = yf / inv; theta = arc / R; rho = R + side d (d: the depth behind the
 *   fine pixel, as pcp_ortho_texture finds it; the interpolation does not wrap across the seam); rho <= 0: no surface (status 0);
 *   p = (float)(c + ((rho cos theta) e + (rho sin theta) b + hh a)), sine and cosine by one fixed sequence of fp64 operations.
 * Reads the map, the depth maps and the keyframe images, writes none of them.  Kernel time under PCP_K_MISC.
 * pcp_ortho_texture_points_cyl_host: pcp_ortho_texture_points_host under a cylinder's frame (host only; out_ok 0 and xyz 0
 * where there is no surface).  pcp_cyl_sincos_host: the sine and cosine of n angles in [0, 64) by that sequence (host only);
 * a negative n, a NULL array or an angle outside [0, 64) or not finite: PCP_ERR_INVALID.  Messages at pcp_last_error(NULL). */
int pcp_ortho_texture_cyl(pcp_context *ctx, const pcp_ortho_texture_params *params, uint8_t *out_rgb, uint8_t *out_mask,
                          uint8_t *out_status, int16_t *out_view, uint8_t *out_count, int64_t out_counts[4]);
int pcp_ortho_texture_points_cyl_host(const pcp_cyl_frame *frame, const pcp_ortho_texture_params *params, const int32_t *source,
                                      const float *depth, float *out_xyz, uint8_t *out_ok);
int pcp_cyl_sincos_host(int64_t n, const double *theta, double *out_sin, double *out_cos);

/* ---- surface defects on ortho maps (no counterpart in the reference) ------------------------------------------------ */
/* The depth layer of a finished map is the deviation of the surface from the frame's own surface: the plane of a facet's
 * frame, or the fitted cylinder of an unrolled map.  This stage turns it into a signed deviation image against a local
 * reference surface, the pixels beyond a threshold into 8-connected regions of one class, and every kept region into one row
 * of integers ("Surface defects on ortho maps", SD1-SD9).  Opt-in: nothing runs unless one of these is called,
 * PCP_ABI_VERSION is unchanged and a caller detects support by the symbols.  Kernels are timed under PCP_K_MISC.  The map is
 * never modified.
 *   params    threshold in metres, finite, 2^-20 <= t <= 1; window_px W in 0..1024; refine 0 or 1, and 1 needs W > 0;
 *             min_support >= 1 (read only when W > 0); min_pixels >= 1; classes bit 0 hollows, bit 1 bulges, not 0.  Anything
 *             else: PCP_ERR_INVALID with a message that names the field.  The parameters are checked before the state.
 *   state     a live, finished map of either kind (pcp_ortho_finish); otherwise PCP_ERR_STATE.
 *   pixel     surface iff its status is 1 or 2 and its depth is finite with |depth| <= 512 m; its quantum
 *             q = llrint((double)depth * 2^20); T = llrint((double)threshold * 2^20).  Pixels refused for their depth are
 *             counted and treated as empty.
 *   W = 0     dev = q; hollow (class 1) iff q >= T, bulge (class 2) iff q <= -T.
 *   W > 0     S, n: sum of q and count of the surface pixels in rows r-W..r+W, columns c-W..c+W clipped to the raster (no
 *             wrap across a cylinder's seam); n < min_support: unsupported (class 0, dev 0, counted); else e = q n - S,
 *             dev = e / n truncated, hollow iff e >= T n, bulge iff e <= -T n.
 *   refine    a second pass over the surface pixels whose first-pass class (every class bit on) is 0: a pixel whose second
 *             count reaches min_support takes S, n, e, dev and class from it, any other keeps the first pass's and is
 *             counted.  The classes mask is applied after the last pass.
 *   regions   8-connected pixels of one class; fewer than min_pixels pixels: dropped (region 0; class and dev kept); the kept
 *             ones are numbered 1..N in ascending order of their lowest linear pixel index.
 *   row       16 int64: class, pixels, pixels of status 1, sum |dev|, max |dev|, its pixel (the lowest among equals), col
 *             min, col max, row min, row max, sum col, sum row, open pixels (on the raster's edge, or with a 4-neighbour that
 *             is no surface pixel), first pixel, pixels on the first pass's reference, 0.
 *   out[8]    regions kept, regions dropped, hollow pixels, bulge pixels, unsupported pixels, pixels refused for their depth,
 *             pixels on the first pass's reference, surface pixels.
 * Depth grows away from the viewer in both kinds of frame, so a hollow is material missing and a bulge material towards the
 * viewer.  The library returns integers only: area = pixels gsd^2, volume = sum |dev| 2^-20 gsd^2, depth = max |dev| 2^-20.
 * pcp_ortho_defects_fetch: the H x W layers (each nullable): dev in quanta, class, region id.  pcp_ortho_defects_table: rows
 * first .. first + max_rows - 1 (out_rows16 nullable: *out_rows alone says how many there are from `first`).  The results
 * belong to the live map: replaced by the next pcp_ortho_defects, dropped by pcp_ortho_finish, either begin, pcp_ortho_end and
 * pcp_destroy; a refused call leaves them; without results both fetches are PCP_ERR_STATE.
 * pcp_ortho_defects_host: the same from the depth and status layers of a map (pcp_ortho_fetch / pcp_ortho_host), on the CPU by
 * the same arithmetic (csrc/pcp_ortho_defects.hpp), bit for bit what the device gives; width, height 1..16384 and at most 2^26
 * pixels; outputs nullable but out; at most max_rows rows are written, *out_rows is their whole number.  Messages at
 * pcp_last_error(NULL). */
typedef struct pcp_ortho_defect_params {
  float threshold;     /* metres */
  int32_t window_px;   /* W: 0 = against the frame's own surface */
  int32_t refine;      /* 0 or 1 */
  int32_t min_support; /* surface pixels a window needs */
  int32_t min_pixels;  /* pixels a region needs to be kept */
  int32_t classes;     /* bit 0 hollows, bit 1 bulges */
} pcp_ortho_defect_params;
int pcp_ortho_defects(pcp_context *ctx, const pcp_ortho_defect_params *params, int64_t out[8]);
int pcp_ortho_defects_fetch(pcp_context *ctx, int32_t *out_dev, uint8_t *out_class, int32_t *out_region);
int pcp_ortho_defects_table(pcp_context *ctx, int64_t first, int64_t max_rows, int64_t *out_rows16, int64_t *out_rows);
int pcp_ortho_defects_host(int32_t width, int32_t height, const float *depth, const uint8_t *status,
                           const pcp_ortho_defect_params *params, int64_t out[8], int32_t *out_dev, uint8_t *out_class,
                           int32_t *out_region, int64_t *out_rows16, int64_t max_rows, int64_t *out_rows);

/* ---- precondition of the match-back(PointCloudProcessor.cpp:480-482,571) ------------------------------- */
/* Number of map points that have ANOTHER map point closer than `radius` (fp32 squared distance, strict <, as
 * kdtree.radiusSearch compares).  The reference credits a visible sample to every map point within 1e-5 m of the
 * sample's fp32 world position; PCP_MATCH_ROUNDTRIP / _IDENTITY credit the sample's own point only, PCP_MATCH_RADIUS
 * credits every such point.  ROUNDTRIP agrees with the reference when no two map points can both lie within 1e-5 m of
 * one sample: call this with radius = 2.5e-5 (the match radius plus twice the largest fp32 round-trip error measured
 * on maps within +-50 m) and expect 0; a non-zero count (duplicated or near-duplicated points, e.g. un-deduplicated
 * scan accumulations) names how many points may receive a neighbour's samples in the reference and under
 * PCP_MATCH_RADIUS, but not under ROUNDTRIP. */
int pcp_close_pairs(pcp_context *ctx, double radius, int64_t *points_with_close_neighbour);

/* ---- measurement -------------------------------------------------------- */
/* When enabled every kernel launch is bracketed by hipEvents on the context's
 * stream; totals are read back with pcp_timing_get (which synchronises). */
int pcp_timing_enable(pcp_context *ctx, int32_t on);
int pcp_timing_reset(pcp_context *ctx);
int pcp_timing_get(pcp_context *ctx, int32_t kernel_id, double *total_ms, int64_t *launches);
const char *pcp_kernel_name(int32_t kernel_id);
/* diagnostic: fraction of (tile, keyframe) pairs the conservative culling keeps (after pcp_depth_pass) */
int pcp_tile_mask_density(pcp_context *ctx, double *kept_fraction);
/* diagnostic: the (tile, keyframe) masks themselves, tiles x mask_words uint32 (bit f & 31 of word f >> 5); either
 * output may be NULL to query the sizes */
int pcp_tile_masks(pcp_context *ctx, int64_t *tiles, int32_t *mask_words, uint32_t *out_words);
/* diagnostic: the order of the uploaded cloud, out_perm[j] = the input index of the point at sorted place j (n int32; a tile is
 * the 64 consecutive places 64 t .. 64 t + 63, a group 16 consecutive tiles).  Synchronises and copies. */
int pcp_cloud_order(pcp_context *ctx, int32_t *out_perm);
/* diagnostic: the bounds the tile masks are built from, 8 floats per bound: centre x y z and radius of the bounding sphere, then
 * the half-extents hx hy hz of the world-axis box about the same centre and a zero.  *tiles bounds of tiles come first, the
 * (*tiles + 15) / 16 bounds of the groups behind them; either output may be NULL to query the size.  Synchronises and copies. */
int pcp_tile_bounds(pcp_context *ctx, int64_t *tiles, float *out8);
/* diagnostic: share of the points of the last pcp_sor / pcp_cloud_smooth SOR pass that the selection kernel handed
 * to the heap kernel (fewer than mean_k + 1 neighbours within one grid cell, or a crowded boundary bin) */
int pcp_sor_redo_fraction(pcp_context *ctx, double *fraction);
/* diagnostic: the mean distance to the mean_k nearest neighbours of every uploaded point, as the last pcp_sor computed
 * it (the quantity StatisticalOutlierRemoval thresholds; statistical_outlier_removal.hpp [upstream] keeps it private).
 * Valid until the next call that smooths or filters; capacity >= the number of uploaded points. */
int pcp_sor_distances(pcp_context *ctx, int64_t capacity, float *out_distance);
/* diagnostic: the kernels replace three IEEE divisions of the projection (pinhole.hpp:17-18 x/z, y/z in fp64;
 * view_culling.cpp:88 u/14, v/14 in fp32) by shorter sequences that are proven to return the same correctly
 * rounded quotients (pcp_device.hpp).  This runs both forms on the device and counts disagreements:
 * `samples` pseudo-random (x, y, z) float triples (all exponents, z > 0) for the fp64 pair, and EVERY fp32 bit
 * pattern for the division by the configured downsample factor.  Both counts must be 0. */
int pcp_selftest_arithmetic(pcp_context *ctx, int64_t samples, uint64_t seed, int64_t *mismatches_fp64,
                            int64_t *mismatches_fp32);
/* diagnostic: three pieces of a (tile, keyframe) visit run in a shorter form than the reference writes (csrc/pcp_visit_forms.hpp):
 * the distortion with its doublings folded into FMAs, the cell rule with the depth buffer on as four compares against the
 * map size, and the distance score's fp32 square root without the compiler's range scaling.  This runs the written and the
 * short form of each on the device and counts disagreements: `samples` pseudo-random float triples through the projection
 * under the configured coefficients, and EVERY fp32 bit pattern as a quotient of the cell rule (configured cull size and
 * downsample factor) and as the square root's argument.  All three counts must be 0.  short_distortion: 1 when the configured
 * p1, p2 let the short distortion run (0: the kernels keep the written form, and the first count compares it with itself). */
int pcp_selftest_visit_forms(pcp_context *ctx, int64_t samples, uint64_t seed, int64_t *mismatches_uv, int64_t *mismatches_cell,
                             int64_t *mismatches_sqrt, int32_t *short_distortion);
/* diagnostic: under a camera whose k3 is a zero and whose other constants are in a proven range (csrc/pcp_visit_forms.hpp,
 * k3_term_droppable), the batched passes of the default configuration leave the k3 term out of the distortion polynomial.  This runs
 * the written projection and the form those passes run under the configured camera on the device, on `samples` pseudo-random
 * float triples (all exponents, z > 0) and on a grid of extreme ones (depths down to 2^-149 under ordinary, huge and non-finite
 * x, y), and counts the triples whose verdicts of the two truncation rules, cell, pixel or -- where a rule accepts -- (u, v)
 * differ.  The count must be 0.  term_dropped: 1 when the configured camera lets the term go (0: the passes keep it). */
int pcp_selftest_k3_term(pcp_context *ctx, int64_t samples, uint64_t seed, int64_t *mismatches, int32_t *term_dropped);
/* diagnostic: the plane of four stages is the eigenvector of the smallest eigenvalue of a symmetric 3 x 3 matrix, found in
 * closed form (pcl::eigen33) by device-only code that rests on two short fp64 reciprocal sequences (csrc/pcp_eigen33.hpp).  This
 * runs that code on the caller's inputs, one lane per item, and returns what it returns, NaNs and infinities included:
 * n matrices as 6 n doubles in the order xx xy xz yy yz zz -> out_ev[n] (the eigenvalue) and out_vec[3 n] (its unit vector, three
 * NaNs where the cross products of two rows are zero or rounding noise: no plane is defined); m arguments -> out_rcp[m] and out_rsqrt[m] (1 / x and 1 / sqrt(x) to two
 * ulp for normal x with a normal result; zero, a negative argument of the root, infinities and NaN give non-finite values).
 * form 0: the code as the map normals compile it, without floating-point contraction -- which is also how the crack-width
 * plane and the crack tangent are built, so this form stands for those two units as well.  form 1: as the MLS fit compiles it,
 * with contraction.  Needs no camera and no cloud and changes no state of the context.  PCP_ERR_INVALID: another form, a
 * negative count or one above 2^27, a NULL array with a count above 0.  The caller compares with a reference of its own
 * (tests/test_eigen33_gpu.py: mpmath at 50 digits). */
int pcp_selftest_eigen33(pcp_context *ctx, int32_t form, int64_t n, const double *matrices, double *out_ev, double *out_vec, int64_t m,
                         const double *args, double *out_rcp, double *out_rsqrt);

#ifdef __cplusplus
}
#endif
#endif /* PCP_HIP_H */
