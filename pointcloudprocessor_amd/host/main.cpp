// main.cpp -- `PointCloudProcessor` command line on top of libpcp_hip.so.
//
// Same flags, same odometry / PCD inputs, same output files and exit codes as the
// reference binary (PCP/src/main.cpp:7-71, PCP/src/PointCloudProcessor.cpp:1007-1032):
//   --point_cloud_path/-p --odometry_path/-o --images_folder/-i --mask_image_folder/-m
//   --output_path/-t --enableMLS --enableNIDOptimize --enableInitialGuessManual --help/-h
// Every flag, with its range, default, error text and help line, is one row of the table in host/cli_options.hpp; the
// refusals of flag combinations are the ordered list below it.  What follows describes what the flags make the program write.
// Stages kept on the host: odometry parsing (:965-1005), keyframe selection (:1050-1075,
// hpp:151-191), trajectory crop (:92-136), PCD reading / ASCII writing.  Hot path on the
// GPU through pcp_shim.hpp.
//
// Differences (this image has no OpenCV):
//   * images are decoded by host/image_io.hpp: <images_folder><ts>.jpg (baseline JPEG, libjpeg's
//     arithmetic, bit-exact with Pillow / libjpeg-turbo here) and masks <mask_folder><ts>.png;
//     <ts>.ppm / <ts>.pgm are accepted when the .jpg / .png is absent.  A keyframe JPEG the device path supports is
//     only entropy-decoded on the host (jpeg_coefficients) and reconstructed on the GPU (pcp_upload_image_jpeg, the
//     same pixels); any other keyframe file is decoded on the host as before.
//   * the 8-bit BGR->HSV->BGR round trip of generateColorMap (:722-741, Appendix B5) is applied by the
//     library while it packs the decoded image (pcp_set_image_adjust: OpenCV 4.2's integer forward routine
//     exactly, its scalar float backward routine); the NID stage reads the raw pixels, as calibrate.cpp does.
//   * --enableNIDOptimize runs the NID cost on the GPU with a BFGS on SE(3) in place of
//     ceres::Solve (same cost, gradient, domain limits and outer loop; not Ceres' line search).
//   * --enableInitialGuessManual is accepted and rejected with an exception (exit -2): the
//     interactive GUI is out of scope.
//   * --cull zbuffer|hpr|hpr_candidates (new, default zbuffer): which of ViewCulling's two routines decides visibility.
//     zbuffer = view_culling (view_culling.cpp:52-174, the routine north_star names; its call is commented out at :43);
//     hpr = hidden_points_removal (:266-334), the routine the reference binary actually calls (:46), flip + convex
//     hull on the GPU; hpr_candidates = only its candidate filter (:276-288), a frustum cull.
//   * --mlsVoxelSize v, --mlsDilationIterations k, --mlsUpsampling none|slp|vgd (new): the three MLSParameters the reference
//     hard-codes (upsampling VOXEL_GRID_DILATION, 0.001 m, 4 iterations, PointCloudProcessor.cpp:78-81; the defaults here);
//     at 1 mm x 4 every input point becomes up to 729 output points.  slp = SAMPLE_LOCAL_PLANE, the switch's other
//     deterministic method (cloudSmooth.cpp:133-152): a disk of samples per fitted point; --mlsUpsamplingRadius r and
//     --mlsUpsamplingStep s (new) are its slp_upsampling_radius / _stepsize (default 0.05 / 0.01, :74-75).  With --gpus N
//     the slp chain runs on the first GPU (MultiCloudSmooth): the files equal the one-GPU run's.
//   * --gpus N (new, default 1): the map is sharded by point index over N GPUs of this node (pcp_multi.hpp: one
//     process, N contexts, RCCL all-reduce(MIN) of the depth maps over xGMI, images broadcast over xGMI); every
//     output file is identical to the one-GPU run.  The NID refinement sums its joint histograms over the shards
//     (same optimum, last-digit differences in the printed cost); --enableMLS deals the MLS queries / the dilated voxel
//     chunks out over the GPUs (MultiCloudSmooth), the two outlier-removal brackets run on GPU 0.
//   * --smoothColorsRadius r (new, default 0 = off, as in the reference): smoothColorsWithLocalRegion(rgbCloud, r)
//     (PointCloudProcessor.cpp:634-703) between smoothColors and removePointsWithNoColor -- the call the reference has
//     commented out at :597 with r = 0.1.  0 < r <= 1; only cloudInWorldWithRGB.pcd changes.  With --gpus N the gathered
//     colours are smoothed on GPU 0 over the whole map: the files equal the one-GPU run's.
//   * --matchBack roundtrip|radius (new, default roundtrip): how a coloured sample is credited back to map points
//     (PointCloudProcessor.cpp:480-482,571-592).  roundtrip = PCP_MATCH_ROUNDTRIP, the sample's own point when its fp32
//     world round trip finds it; radius = PCP_MATCH_RADIUS, every map point within 10 um of the sample, as the reference's
//     kdtree.radiusSearch does (maps with duplicated points differ).  radius needs the whole map on one GPU: --gpus N > 1
//     with it is rejected.
//   * --fuseMasks 0|1 (new, default 0 = the reference's behaviour; needs --mask_image_folder): 1 = one segmentation label
//     per map point.  The reference appends every keyframe's mask samples to cloudInWorldWithRGBandMask.pcd
//     (PointCloudProcessor.cpp:533-551, 932-947, "TODO: fix it" at :938): every map point once per keyframe that sees it,
//     with conflicting labels.  With 1 that file has exactly the rows, in the order, of cloudInWorldWithRGB.pcd -- the map
//     point's x y z, the same rgb (after --smoothColorsRadius when given; no (255,0,0) override) -- and segmentMask is the
//     label fused on the GPU from the masks of the point's top-5 views (pcp_set_label_fusion; DESIGN.md "Fused segmentation
//     labels"); the host concatenation is not built.  A keyframe whose mask is missing throws "Failed to read image from:
//     <mask path>" (exit -2).  The per-keyframe _rgb-mask.pcd dumps are still written, unless --skip_filtered_dumps 1: the
//     per-keyframe loop is then skipped altogether.  Works with --gpus N and --matchBack radius.
//   * --deviceWriter 0|1 (new, default 0): 1 = the rows of every ASCII PCD the run writes are formatted on the device and
//     downloaded as text (DESIGN.md "Device PCD writer"): the final files and <stem>_mls.pcd from the results resident on the
//     GPU (pcp_colour_compact_ascii, pcp_mls_fetch_ascii; one-shot and --streamColour 1), scans-crop.pcd and the per-keyframe
//     dumps from the arrays those sites hold (pcp_ascii_rows).  Every file is byte for byte the --deviceWriter 0 file; headers,
//     names, messages and exit codes are unchanged.  --gpus N > 1 is refused: the resident forms do not exist on index shards.
//   * --deviceReader 0|1 (new, default 0): 1 = the rows of the ASCII PCDs the run reads -- the map (-p) and, with --enableMLS 1,
//     the crop CloudSmooth reads back (cloudSmooth.cpp:92) -- are parsed on the device (pcp_ascii_parse; DESIGN.md "Device PCD
//     reader"): every float bit for bit the strtof value loadPCDFile returns.  A file the device reader does not take (a row
//     outside plain decimal text, fewer rows than POINTS) is named on stderr with the row and read by the host reader whole;
//     binary and binary_compressed maps ignore the flag.  Messages, exit codes, phase keys and every output file are those of
//     --deviceReader 0.  Works with --gpus N (the first device parses).
//   * --streamColour 0|1 (new, default 0; with --enableMLS 1) and --streamChunk voxels (default 2^28): 1 = the smoothed cloud
//     is never gathered on the host.  The smoothing chain runs in its streamed form and every chunk of it is handed, on the
//     device, to the colour stage (CloudSmooth::processAndColorizeStreamed; DESIGN.md "Streamed colourisation"): one sweep
//     merges the chunks' depth maps, a second colours every chunk against the merged maps.  scans-crop_mls.pcd,
//     cloudInWorldWithRGB.pcd and, with --fuseMasks 1, cloudInWorldWithRGBandMask.pcd are written chunk by chunk and are byte
//     for byte the files of a --streamColour 0 run; a smoothed cloud of more rows than one upload takes (the reference's
//     1 mm x 4 on a real map) can only be coloured this way.  One GPU, the z-buffer routine; the per-keyframe dumps, the NID
//     stage, --matchBack radius, --smoothColorsRadius and masks without --fuseMasks 1 need the whole cloud and are refused.
//   * --balanceExposure 0|1 (new, default 0 = the reference's behaviour): 1 = one brightness gain per keyframe, estimated on
//     the GPU from the map points that two keyframes both colour (DESIGN.md "Exposure gains"; the reference has one hand-set
//     brightness, PointCloudProcessor.cpp:726-729, and balancing scripts that are run over the keyframe folder beforehand).
//     The colour stage then runs depth pass, colour pass over all keyframes, the pair statistics and the solve, and a
//     finalise that applies the gains; <outputPath>exposure_gains.txt lists "<imageTimestamp> <gain>" per keyframe.  Only
//     cloudInWorldWithRGB.pcd (and the rgb of a --fuseMasks 1 file) changes: the per-keyframe dumps keep the sampled colours.
//     --gpus N above 1 and --streamColour 1 are refused: the statistics are additive over shards and chunks, but that
//     exchange is not built.
//   * --outputLeaf L (new, default 0 = off; 1e-4 <= L <= 1) and --skip_full_cloud 0|1 (new, default 0): with L > 0 the run also
//     writes <outputPath>cloudInWorldWithRGB_voxel.pcd -- one XYZRGB row per occupied voxel of edge L of the coloured cloud:
//     the centroid and the mean colour of the voxel's rows, in pcl::VoxelGrid's leaf order on a lattice anchored at the world
//     origin -- and, with --fuseMasks 1, <outputPath>cloudInWorldWithRGBandMask_voxel.pcd with the mean fused label as
//     segmentMask.  The reduction runs on the GPU over the colour result where it lies (pcp_voxel_reduce_*; DESIGN.md
//     "Voxel-grid output"), after --smoothColorsRadius when given; in the one-shot path and under --streamColour 1, where
//     every chunk is added after it is coloured, the files are byte for byte the same.  It is what pcl::VoxelGrid /
//     voxelgrid_sampling (frame_cpu.cpp:360-451) users run over the full file afterwards.  --skip_full_cloud 1 (needs
//     --outputLeaf): cloudInWorldWithRGB.pcd / cloudInWorldWithRGBandMask.pcd are neither fetched nor written; under
//     --streamColour 1 the chunks are then compacted with capacity 0, so only the voxel rows leave the device.  --gpus N
//     above 1 is refused: the voxel sums of the index shards would have to be added across GPUs, which is not built.  The
//     voxel files are small and always go through the host writer, --deviceWriter 1 or not.
//   * --geometryMaps 0|1 (new, default 0) and --normalRadius r (new, default 0.1; 0 = no normals): with 1, every selected
//     keyframe also writes <outputPath>geometry_maps/<imageTimestamp>_range.npy, _xyz.npy, _normal.npy and _index.npy -- the
//     distance_mask, points_3d_mask and norm_mask that scripts/genNormAndDistanceMask.py (generate_norm_masks :200-231,
//     generate_distance_masks :233-266) scatters from filtered_pcd/ afterwards, at camera resolution, plus the index of the
//     map point behind every pixel (NumPy format 1.0, little-endian <f4 / <i4, C order: (H, W), (H, W, 3), (H, W, 3),
//     (H, W); empty pixels hold 0, index -1).  They are made on the GPU (pcp_estimate_normals once, pcp_frame_geometry per
//     keyframe; DESIGN.md "Geometry maps") from the raw map, with the poses the colourisation uses (after the NID
//     stage), by the configured cull: the nearest kept point wins a pixel, and the normals come from the whole map within
//     --normalRadius (0.005 <= r <= 1) instead of from each keyframe's culled cloud.  --normalRadius 0 writes no _normal
//     file.  No other output changes.  --gpus N above 1 is refused (an index shard sees only its own points; the per-pixel
//     keys of the shards would have to be merged across GPUs, which is not built), and so is --enableMLS 1 (the colour
//     stage then holds the smoothed cloud; maps of it are not built).
//   * --crackMaps 0|1 (new, default 0; needs --mask_image_folder) and --crackThreshold t (new, default 0, 0..255): with 1,
//     every selected keyframe also writes <outputPath>crack_maps/<imageTimestamp>_edt2.npy (<u4, (H, W)) and _nearest.npy
//     (<i4, (H, W)) -- what scripts/genNormAndDistanceMask.py preprocess() :150-198 computes on the host with cv2.threshold
//     :167 and scipy.ndimage.distance_transform_edt :168: the exact SQUARED distance from every pixel of the keyframe's mask
//     to the nearest pixel whose mask byte is <= t (sqrt of it as fp64 is scipy's value bit for bit), and that pixel's
//     linear index y * W + x, the lowest among equally near ones; a mask without such a pixel holds 0xFFFFFFFF and -1.  Made
//     on the GPU from the masks the colour stage uploads (pcp_mask_edt_frames; DESIGN.md "Mask distance maps").  A keyframe
//     whose mask could not be read writes no files.  No other output changes.  --gpus N above 1 is refused (one context
//     holds every mask: the shards would add nothing).
//   * --crackWidth 0|1 (new, default 0; needs --mask_image_folder) and --crackPlaneRadius R (new, default 150, 1..181;
//     --crackThreshold is reused): with 1, every selected keyframe whose mask was read also writes
//     <outputPath>crack_width/<imageTimestamp>_width.npy (<f4, (H, W), metres), _edges.npy (<i4, (H, W, 4): the near and the
//     far edge point of the pixel, doubled, -1 = missing), _flags.npy (|u1, (H, W): SITE CENTRE NEAR FAR PLANE RAYS WIDTH from
//     bit 0) and _points.npy (<f4, (H, W, 6): the two 3-D edge points in camera coordinates) -- the second half of
//     Crack.process() in scripts/genNormAndDistanceMask.py, compute_skeleton_edge_pts :396-478, for EVERY foreground pixel of
//     the mask instead of hand-picked skeleton points: the edges along the exact EDT direction (for trace_edge :706-762), the
//     plane of the position image's window of +-R pixels (find_local_plane :601-636) and the intersection of the edge rays
//     with it (for the grid search of search_3d_edge_points :564-599).  Made on the GPU from the masks the colour stage
//     uploads and the raw map (pcp_crack_width; DESIGN.md "Crack width maps"), with the poses the colourisation uses.  The
//     counts of sites and widths are printed per keyframe.  No other output changes.  --gpus N above 1 and --enableMLS 1 are
//     refused for the reasons --geometryMaps gives.
//   * --crackFuse 0|1 (new, default 0; needs --mask_image_folder), --crackLinkRadius r (new, default 0.02, 0.005..1) and
//     --crackMinViews v (new, default 1, 1..4096; --crackThreshold and --crackPlaneRadius are reused): with 1, after the
//     colour stage, the widths of every selected keyframe whose mask was read are brought back to the map points that see them
//     and the run writes <outputPath>crack_width/map_width.npy (<f4, (n): the mean width in metres over the keyframes that
//     credit the point, 0 without one), map_width_best.npy (<f4, (n): the width from the nearest such keyframe), map_views.npy
//     (<u4, (n): their number), map_crack.npy (<i4, (n): the id of the point's crack, -1 for a point outside every crack) and
//     cracks_3d.json: one record per crack -- the connected components, under the link radius, of the points with v credited
//     keyframes or more -- with id, points, centre_points, width_mean_mm / width_min_mm / width_max_mm and box_min / box_max.
//     n is the map's point count, input order.  This is what the per-point records of compute_skeleton_edge_pts (:396-478) and
//     the result file crack_width_3d_results.json (:476-478) hold for hand-picked pixels, for the whole map and with the
//     cracks told apart.  Made on the GPU (pcp_crack_fuse_*, pcp_crack_components; DESIGN.md "Crack widths on the map").
//     With --crackWidth 1 as well a keyframe's width stage runs twice.  No other output changes.  --gpus N above 1 and
//     --enableMLS 1 are refused for the reasons --geometryMaps gives.
//   * --crackLength 0|1 (new, default 0; needs --crackFuse 1 and is refused where that is): with 1 the run also writes
//     <outputPath>crack_width/map_crack_pos.npy (<u8, (n): the point's arc position along its crack from the crack's end a, in
//     units of 2^-20 m; 2^64 - 1 for a point outside every crack), crack_paths.npy (<i4: the cracks' centrelines one after the
//     other, input indices from end a to end b), crack_path_offsets.npy (<i8, (cracks + 1): where each crack's centreline
//     starts in it) and crack_lengths_3d.json: one record per crack, the cracks and order of cracks_3d.json, with id,
//     length_m (the geodesic length between the ends over the links of the crack), hops, end_a, end_b, end_a_xyz, end_b_xyz and
//     path_width_mean_mm / path_width_min_mm / path_width_max_mm over the fused widths of the centreline's points.  The
//     reference's script orders a crack only by a 2-D skeleton per keyframe.  Made on the GPU (pcp_crack_lengths; DESIGN.md
//     "Crack lengths on the map").  cracks_3d.json and every other output stay as they are.
//   * --crackSkeleton 0|1 (new, default 0; needs --crackFuse 1 and is refused where that is) and --crackSkeletonStep s (new,
//     metres, default 0 = twice the link radius; at least the link radius, at most 16): with 1 the run also writes
//     <outputPath>crack_width/map_crack_node.npy (<i4, (n): the id of the point's node of its crack's skeleton, -1 for a point
//     outside every crack), crack_nodes.npy (<i8, (nodes, 10): crack_row, band, points, sum_w, min_w, max_w, sum_qx, sum_qy,
//     sum_qz, degree) with crack_node_ids.npy (<i4, (nodes)), crack_edges.npy (<i8, (edges, 3): u, v, links) and
//     crack_skeleton_3d.json: one record per crack, the cracks and order of cracks_3d.json, with id, nodes, edges, ends,
//     junctions, loops, skeleton_length_m and the centroids of its end and junction nodes (end_xyz, junction_xyz).  The
//     reference's script skeletonises each keyframe's mask in 2-D (preprocess(): pcv.morphology.skeletonize).  Made on the GPU
//     (pcp_crack_skeleton; DESIGN.md "Crack skeletons on the map").  Every other output stays as it is.
//   * --crackDirection 0|1 (new, default 0; needs --crackFuse 1 and is refused where that is) and --crackUp x,y,z (new, default
//     0,0,1: finite, not zero, normalised in fp64): with 1 the run also writes <outputPath>crack_width/map_tangent.npy (<f4,
//     (n, 3): the unit direction of the point's crack at the point, from the covariance of its links, its largest component
//     positive; zeros for a point with fewer than two links or outside every crack), map_anisotropy.npy (<f4, (n): 1 where the
//     links lie on a line, about 1/2 on a flat patch, 0 without a tangent) and crack_directions_3d.json: one record per crack,
//     the cracks and order of cracks_3d.json, with id, links (ordered: every link counts from both ends), axis (the unit
//     direction of the whole crack, zeros when it has none), anisotropy, inclination_deg = acos|axis . up| (0..90) and class:
//     vertical below 22.5, horizontal above 67.5, else diagonal; none without an axis.  With --facets 1 also facet (as in
//     cracks_3d.json), facet_kind (plane, cylinder, none), for a plane out_of_plane_deg = asin|axis . normal|, and for a
//     cylinder --facetCylinders 1 fitted to_axis_deg = acos|axis . a| with cylinder_class: longitudinal below 22.5,
//     circumferential above 67.5, else diagonal.  The reference only blurs one keyframe's 2-D skeleton and shows it
//     (scripts/evalSkeletonDirection.py).  Made on the GPU (pcp_crack_directions; DESIGN.md "Crack directions on the map").
//     Every other output stays as it is.
//   * --crackBranches 0|1 (new, default 0; needs --crackFuse 1 and is refused where that is) and --crackPrune p (new, metres,
//     default twice the skeleton's band width; 0 .. 1024): with 1 the run also makes the skeleton (--crackSkeletonStep; not its
//     files unless --crackSkeleton 1 asks) and writes <outputPath>crack_width/map_crack_branch.npy (<i4, (n): the id of the
//     point's branch, -1 outside every crack, -2 on a kept junction, -3 on a pruned spur), crack_branches.npy (<i8, (rows, 15):
//     crack_row, nodes, edges_inside, attachments, junction_u, junction_v, points, sum_w, min_w, max_w, pos_min, pos_max, sum_qx,
//     sum_qy, sum_qz) with crack_branch_ids.npy (<i4, (rows)), crack_branch_moments.npy (<i8, (rows, 20)) and
//     crack_branches_3d.json: one record per crack, the cracks and order of cracks_3d.json, with id, branch_count (the
//     table's word `branches`: the key is the list's), bridges, junctions_kept, ends_kept, pruned_branches, pruned_nodes,
//     pruned_points, kept_length_m and the list branches: per branch id,
//     points, length_m, mean_width, min_width, max_width (metres), arc_from_m, arc_to_m (where along the crack it lies),
//     attachments, centroid and the direction fields of crack_directions_3d.json for the branch's own axis (axis, anisotropy,
//     inclination_deg, class against --crackUp; with --facets 1 the crack's facet, facet_kind, out_of_plane_deg, and on a fitted
//     cylinder to_axis_deg and cylinder_class).  The reference never takes a skeleton apart.  Made on the GPU
//     (pcp_crack_branches; DESIGN.md "Crack branches on the map").  Every other output stays as it is.
//   * --balanceImages 0|1 (new, default 0 = the reference's behaviour), --claheClip c (new, default 1.0; 0 = no clipping),
//     --claheTiles x,y (new, default 8,8, each 1..16) and --balanceGamma g (new, default 0.8; 1 = identity table): with 1,
//     every keyframe is colour-balanced on the GPU as it is uploaded -- CLAHE on a lightness channel, then a gamma table --
//     which the reference does beforehand by running scripts/image_color_balance_autonomous.py (clip 1.0, gamma 0.8: the
//     defaults here) or scripts/image_color_balance.py (--claheClip 3 --balanceGamma 1.1) over the keyframe folder and
//     pointing -i at the rewritten JPEGs (pcp_set_image_balance; DESIGN.md "Image balance").  Two stated differences: the
//     lightness channel is V of the 8-bit HSV conversion generateColorMap uses, not L of 8-bit Lab, and the balanced
//     pixels are never re-encoded as JPEG.  The balance comes before generateColorMap's HSV round trip, and the NID stage
//     sees the balanced keyframes too, as it does when the folder was balanced.  The three value flags without
//     --balanceImages 1 are errors.  Works with every cull and match mode, --gpus N (every GPU balances its own copy of the
//     same pixels), --streamColour 1, --balanceExposure 1 and the device JPEG path.
//   * --orthoDefects 0|1 (new, default 0; needs --orthoMap 1, refused by name without it and with --gpus N above 1) with
//     --defectThreshold t (default 0.002 m, 2^-20..1), --defectWindow W (default 0 pixels, 0..1024; 0: against the frame's own
//     surface), --defectRefine 0|1 (default 0; needs W > 0), --defectMinSupport k (default 1), --defectMinPixels k (default 1)
//     and --defectClasses hollow|bulge|both (default both), each refused by name without --orthoDefects 1: beside the other
//     layers of ortho/ and of every ortho/facet_<row>/ (planar and unrolled) the run writes ortho_defect_dev.npy (<i4: the
//     signed deviation in quanta of 2^-20 m), ortho_defect_class.npy (|u1: 0, 1 hollow, 2 bulge), ortho_defect_region.npy (<i4:
//     0, or the region's id) and defects.json (the parameters, the eight counts, and per kept region its kind, pixels, area_m2,
//     volume_m3, depth_m and its pixel, box, centroid, measured_fraction, open_pixels, first_pass_pixels and the raw row of 16
//     integers; numbers as %.9g).  No counterpart in the reference.  Made on the GPU (pcp_ortho_defects; DESIGN.md "Surface
//     defects on ortho maps").  Without the flag every file is byte for byte what it was.
//   * --orthoMap 0|1 (new, default 0), --orthoGsd g (new, default 0.01, metres per pixel, 1e-4..1), --orthoFill R (new, default
//     0, pixels, 0..1024) and --orthoFrame auto|ox,oy,oz,ux,uy,uz,vx,vy,vz (new, default auto): with 1 the run also writes one
//     orthographic picture of the coloured cloud, <outputPath>ortho/ortho_rgb.npy (|u1, (H, W, 3)), ortho_depth.npy (<f4,
//     (H, W): the depth along the viewing direction, 0 on an empty pixel), ortho_index.npy (<u4, (H, W): the row of the
//     coloured cloud's point behind the pixel -- of the map, or of the smoothed cloud with --enableMLS 1 -- 0xFFFFFFFF on an
//     empty pixel), ortho_status.npy (|u1: 0 empty, 1 direct, 2 filled from the nearest occupied pixel within R) and
//     ortho_frame.json (o, u, v, n, gsd, width, height, d_min, d_max: pixel (col, row) at depth d is the world point
//     o + (col + 0.5) gsd u + (row + 0.5) gsd v + d n).  With --fuseMasks 1 also ortho_label.npy (|u1), with --crackFuse 1
//     also ortho_width.npy (<f4: map_width.npy[index]) and ortho_crack.npy (<i4: map_crack.npy[index], -1 on an empty pixel).
//     auto: the plane fitted to the finite points of the map the run read (with --enableMLS 1: of the crop the chain
//     smooths), seen from the side of the mean keyframe position; nine numbers: origin, image x and image y axes as given,
//     n = u x v, the raster sized to hold the map's points on the positive side of the origin, the depth window unbounded.
//     The reference stops at per-keyframe perspective pictures (visualize_skeleton_edge_pts, save_results of
//     scripts/genNormAndDistanceMask.py).  Made on the GPU (pcp_ortho_*; DESIGN.md "Orthographic maps"); works with
//     --enableMLS 1 and with --enableMLS 1 --streamColour 1, where the chunks are added as they are coloured.  No other output
//     changes.  --gpus N above 1 is refused (the shards' key images would merge by an all-reduce(MIN), which is not built).
//   * --orthoTexture k (new, default 0 = off, 1..16), --orthoTextureViews m (new, default 1, 1..5), --orthoTextureInterp 0|1 (new,
//     default 1) and --orthoTextureStep s (new, default 0.05, metres): with --orthoMap 1 the run also writes the orthophoto of
//     that map, k fine pixels per map pixel and axis, coloured straight from the keyframe images instead of from one map point
//     per pixel: <outputPath>ortho/ortho_photo_rgb.npy (|u1, (H k, W k, 3)), ortho_photo_mask.npy (|u1: the crack mask of the best
//     view at image resolution, 0 without masks), ortho_photo_view.npy (<i2: the keyframe of the best view, -1 where nothing is
//     textured), ortho_photo_status.npy (|u1: 0 no surface, 1 textured, 2 surface no keyframe sees) and ortho_photo.json (scale,
//     views, interpolate, max_step, the fine gsd, width, height and the counts).  m = 1 takes the sharpest view, m = 5 the
//     reference's weighted mean of five.  A raster of more than 2^28 fine pixels is textured in bands of map rows.  Made on the
//     GPU (pcp_ortho_texture; DESIGN.md "Orthophotos"); works in the one-shot and in the --streamColour 1 form, where it runs
//     after the last chunk on the merged depth maps.  The other ortho files are byte for byte what they are without the flag.
//     Refused: without --orthoMap 1, with --gpus N above 1 and with --cull hpr / hpr_candidates (no depth maps to test a
//     surface point against); the three value flags without --orthoTexture are errors.
//   * --facets 0|1 (new, default 0), --facetRadius r (new, default 0.1, 0.005..1), --facetAngle deg (new, default 10, 0..45),
//     --facetPlaneTol m (new, default 0.01, 1e-4..0.1), --facetMaxCurvature c (new, default 0.02, 0..1), --facetMinPoints k (new,
//     default 1000, 1..2^24), --facetMaxRms m (new, default 0.01) and --normalRadius as above (not 0): with 1 the run also
//     partitions the map into the faces of the structure and writes <outputPath>facets/facet_label.npy (<i4, one per map point:
//     the id of the point's facet -- the lowest row among its points -- or -1) and facets.json (per facet id, points, centroid,
//     normal, rms, planar, box_min, box_max; numbers as %.9g).  Two points share a facet when a chain of links joins them: closer
//     than r, normals within the angle, each within the plane tolerance of the other's tangent plane; a facet is planar when
//     the rms distance of its points to its own plane is at most --facetMaxRms.  With --orthoMap 1 --orthoFrame facets the run
//     writes one directory <outputPath>ortho/facet_<row>/ per planar facet (row: its place in facets.json), each holding what
//     ortho/ holds otherwise, on a frame fitted to the facet's own points and drawn from the facet's own points only; there is
//     no whole-map ortho/ortho_*.npy then (and no ortho_width / ortho_crack layer).  With --crackFuse 1 every crack of
//     cracks_3d.json gains "facet", the most frequent facet id among its points (ties to the lowest id, -1 when none has
//     one); without --facets 1 the file is byte for byte what it was.  Made on the GPU (pcp_facets, pcp_ortho_add_facet;
//     DESIGN.md "Planar facets").  Refused: --gpus N above 1, --enableMLS 1, --streamColour 1, --normalRadius 0, and
//     --orthoFrame facets without --facets 1.
//   * --facetCylinders 0|1 (new, default 0; needs --facets 1): with 1 every facet that is not planar is fitted a cylinder from
//     its points and their normals (closed form: the axis from the normals' scatter, the algebraic circle across it); every
//     record of facets.json gains "kind" (0 neither, 1 planar, 2 cylindrical: fitted with an rms of rho - R of at most
//     --facetMaxRms) and, where the fit succeeded, "cylinder" (c, a, e, b, radius, gsd, width, height, d_min, d_max, side, rows,
//     rms, dev_min, dev_max, arc, eigenvalues; numbers as %.9g).  With --orthoMap 1 --orthoFrame facets the run writes one
//     directory ortho/facet_<row>/ per cylindrical facet too: the facet unrolled along its arc, x along the arc and y along
//     the axis at --orthoGsd metres per pixel both ways, the depth layer the radial deviation from the cylinder; its
//     ortho_frame.json carries "kind": "cylinder" and the cylinder's frame.  Under --orthoTexture k the planar facets are
//     textured and each cylindrical one is named on stderr as skipped.  Without the flag every file is byte for byte what it
//     was.  Made on the GPU (pcp_ortho_begin_cyl; DESIGN.md "Cylindrical facets").
//   * --orthoTextureCylinders 0|1 (new, default 0; needs --orthoTexture k, --facetCylinders 1 and --orthoFrame facets, refused by
//     name without any of them): with 1 every cylindrical facet's directory gains ortho_photo_rgb / mask / view / status.npy and
//     ortho_photo.json in the planar facets' format, banded the same way, and no facet is named as skipped.  Made on the GPU
//     (pcp_ortho_texture_cyl; DESIGN.md "Orthophotos of unrolled maps").  Without the flag every file, byte and message is what
//     it was.
//   * --compareMap base.pcd (new, default none), --compareRadius rc (new, default 0.03, at least 0.005), --compareDepth L (new,
//     default 0.05, at least 0.005; sqrt(rc^2 + L^2) at most 0.5), --compareMinPoints k (new, default 5, at least 2),
//     --compareRegError e (new, default 0, metres) and --normalRadius as above (not 0): the run also compares the map with the
//     earlier survey in base.pcd and writes <outputPath>compare/distance.npy (<f4, one per map point: the signed distance in
//     metres along the point's normal, turned towards the mean keyframe position, from the base's surface to the map's inside a
//     cylinder of radius rc and half length L; positive: deposit, bulge, movement towards the viewer), lod.npy (<f4: the level of
//     detection, 1.96 standard errors of the difference plus e), status.npy (|u1: 0 no core point, 1 no counterpart in the base,
//     2 too few map points, 3 measured and within lod, 4 significant positive, 5 significant negative) and compare.json (the
//     parameters, the eight counts of pcp_compare, and the number, mean and extremes of the significant distances; numbers as
//     %.9g).  With --orthoMap 1 every map directory (ortho/, ortho/facet_<row>/) gains change.npy (<f4: distance.npy[index], 0
//     on an empty pixel) and change_status.npy (|u1: status.npy[index]).  Base points the map has no counterpart for (surface
//     that disappeared) are found by a second run with the two files swapped.  Made on the GPU (pcp_compare; DESIGN.md "Map
//     comparison").  Refused: --gpus N above 1, --enableMLS 1, --streamColour 1, --normalRadius 0.  Without the flag every file,
//     byte and message is what it was.
//   * --compareRegister 1 (new, default 0; needs --compareMap), --registerRadius r (new, default 0.05, 0.005..0.5),
//     --registerMaxDistance d (new, default 0.02, above 0 and at most r), --registerStride k (new, default 1) and
//     --registerIterations i (new, default 20, 1..1000): before the comparison the base is brought onto the map by point-to-plane
//     ICP under the map's normals, and the run also writes <outputPath>compare/registration.json (the 4 x 4 base -> map, the
//     parameters, the log with one row per iteration -- pairs, rms, dof, the update's rotation and shift in metres --, the
//     status -- 0 converged, 1 iteration limit, 2 too few pairs --, and the pairs, dof and rms of the last iteration; numbers
//     as %.17g) and compare/base_transform.txt (four rows of %.17g).  The rms is what --compareRegError may be given in a second
//     run; nothing applies it.  Made on the GPU (pcp_compare_register; DESIGN.md "Map registration").  Refused: the flag
//     without --compareMap, and with it what --compareMap refuses.  Without the flag every file, byte and message is what it was.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <malloc.h>
#include <map>
#include <memory>
#include <sstream>
#include <thread>
#include <exception>
#include <mutex>
#include <condition_variable>

#include "cli_options.hpp"
#include "image_io.hpp"
#include "pcd_io.hpp"
#include "pcp_multi.hpp"
#include "pcp_shim.hpp"
#include "pcd_device_reader.hpp"

namespace fs = std::filesystem;
using namespace pcp_amd;

// Wall-clock split of a run (PCP_CLI_TIMING=<file>: one JSON object, seconds): where the time of the command line goes --
// the reference has no such report; `bench.py`'s cli_e2e leg reads it (at scale the ASCII I/O dominates).
struct PhaseClock {
  std::vector<std::pair<std::string, double>> phases;
  std::mutex mu;
  using clock = std::chrono::steady_clock;
  static double since(clock::time_point t0) { return std::chrono::duration<double>(clock::now() - t0).count(); }
  void add(const std::string &name, double s) {
    std::lock_guard<std::mutex> lk(mu);
    for (auto &p : phases)
      if (p.first == name) {
        p.second += s;
        return;
      }
    phases.emplace_back(name, s);
  }
  void write(const char *path, double total) {
    std::ofstream f(path);
    f << "{";
    for (const auto &p : phases) f << "\"" << p.first << "\": " << p.second << ", ";
    f << "\"total\": " << total << "}\n";
  }
};
static PhaseClock g_clock;
struct Phase {  // adds its lifetime to a named phase
  std::string name;
  PhaseClock::clock::time_point t0 = PhaseClock::clock::now();
  explicit Phase(const char *n) : name(n) {}
  ~Phase() { g_clock.add(name, PhaseClock::since(t0)); }
};

struct Frame {  // FrameData (PCP/include/FrameData.hpp:89-126)
  std::string imagePath, maskImagePath;
  double imageTimestamp = 0;
  pcp_pose pose{};
};

class Processor {
 public:
  explicit Processor(const Options &o) : opt(o), enableMaskSegmentation(!o.maskImageFolder.empty()) {}
  ~Processor() {
    stopDecoders();
    if (device_thread.joinable()) device_thread.join();
  }

  void process() {  // PointCloudProcessor::process, PointCloudProcessor.cpp:1007-1032
    // The GPU context takes a quarter of a second to come up (HIP runtime, code objects, queues): it is created on a thread of
    // its own while this one reads the odometry and the map and writes the crop, and the keyframes' decoders start as soon as
    // the keyframes are known -- by the time the device is ready the first images wait decoded (end to end, 1 M points x 32
    // keyframes from a tmpfs: 0.60 -> 0.42-0.43 s without the per-keyframe dumps, 0.69 -> 0.48 s with them; profiles/r05b_cli_e2e_probe.log).  Same calls in the same order on this thread.
    device_thread = std::thread([this]() {
      try {
        gpu.reset(new MultiDevice(opt.gpus));
      } catch (...) {
        device_error = std::current_exception();
      }
    });
    loadImagesAndOdometry();
    loadPointCloud();
    generateResultStorageFolder();
    selectKeyframes();
    if (!opt.enableNIDOptimize) startDecoders();  // (with the NID stage the first consumer wants the images unadjusted and again later: decoded on demand)
    setupDevice();
    if (opt.stream_colour) {
      streamedColourisation();
      return;
    }
    if (!opt.skip_filtered_dumps) viewCullingAndSaveFilteredPcds();
    if (opt.enableNIDOptimize)
      applyNIDBasedPoseOptimization();
    else if (opt.enableInitialGuessManual)
      throw std::runtime_error("the manual initial-guess GUI is not part of this build");
    if (opt.geometry_maps) writeGeometryMaps();  // (with the poses the colourisation is about to use)
    pcdColorizationAndSmooth();
  }

 private:
  Options opt;
  bool enableMaskSegmentation;
  std::vector<Frame> frames, keyframes;
  XYZICloud cloud;
  std::unique_ptr<MultiDevice> gpu;
  std::thread device_thread;
  std::exception_ptr device_error;
  int img_w = 0, img_h = 0;
  bool images_uploaded = false, images_adjusted = false;
  std::vector<uint8_t> mask_missing;
  std::vector<double> T_camera_lidar_optimized;
  pcp_mls_params mls_params{};  // --streamColour 1: the chain's parameters, kept for streamedColourisation
  std::vector<float> ortho_fit_xyz;    // --orthoMap 1 with --enableMLS 1 (one-shot): the crop the chain smoothed, for the frame
  std::vector<uint32_t> ortho_index;   // --orthoMap 1: the index layer, for the crack layers --crackFuse 1 adds
  MapComparison compare_;              // --compareMap: the per-point result, for the maps' change layers
  Registration registration_;          // --compareRegister 1: what was written to compare/registration.json
  Facets facets_;                      // --facets 1: the partition, for the per-facet maps and the cracks' "facet"
  std::vector<uint8_t> facet_kind_;    // --facetCylinders 1, per facet: 0 neither, 1 planar, 2 cylindrical
  std::vector<pcp_cyl_frame> facet_cyl_;  // --facetCylinders 1, per facet: the fitted cylinder's frame at --orthoGsd (where the fit succeeded)
  std::vector<float> map_normals_;     // --facetCylinders 1: the map normals the cylinders are fitted from (3 per point)
  pcp_ortho_frame ortho_frame_used{};

  void loadImagesAndOdometry() {  // :965-1005
    Phase ph("odometry_s");
    std::ifstream vo(opt.odometryPath);
    std::string line;
    while (std::getline(vo, line)) {
      std::istringstream iss(line);
      double ts, x, y, z, qw, qx, qy, qz;
      if (!(iss >> ts >> x >> y >> z >> qw >> qx >> qy >> qz)) break;  // stop at the first malformed line
      Frame f;
      f.pose = {x, y, z, qw, qx, qy, qz};
      f.imageTimestamp = ts;
      const std::string stem = opt.imagesFolder + std::to_string(ts);  // "%f": 6 decimals (:981)
      f.imagePath = stem + ".jpg";
      if (!fs::exists(f.imagePath)) f.imagePath = stem + ".ppm";
      if (!fs::exists(f.imagePath)) continue;  // skip this frame if its image does not exist (:984-987)
      if (enableMaskSegmentation) {
        f.maskImagePath = opt.maskImageFolder + std::to_string(ts) + ".png";  // :991
        if (!fs::exists(f.maskImagePath) && fs::exists(opt.maskImageFolder + std::to_string(ts) + ".pgm"))
          f.maskImagePath = opt.maskImageFolder + std::to_string(ts) + ".pgm";
      }
      frames.push_back(f);
    }
  }

  void loadPointCloud() {  // :92-154
    double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {DBL_MIN, DBL_MIN, DBL_MIN};  // DBL_MIN: sic (B10)
    for (const auto &f : frames) {
      const double p[3] = {f.pose.x, f.pose.y, f.pose.z};
      for (int a = 0; a < 3; ++a) {
        mn[a] = std::min(mn[a], p[a]);
        mx[a] = std::max(mx[a], p[a]);
      }
    }
    for (int a = 0; a < 3; ++a) {
      mn[a] -= 2.0;
      mx[a] += 2.0;
    }
    XYZICloud original;
    {
      Phase ph("pcd_read_s");
      if (readPCD(opt.pointCloudPath, original) == -1) throw std::runtime_error("Couldn't read point cloud file.");
    }
    std::cout << "Start crop pcd..." << std::endl;
    // pcl::CropBox with Vector4f(min), Vector4f(max): keep min <= p <= max (fp32 bounds)
    const float fmn[3] = {static_cast<float>(mn[0]), static_cast<float>(mn[1]), static_cast<float>(mn[2])};
    const float fmx[3] = {static_cast<float>(mx[0]), static_cast<float>(mx[1]), static_cast<float>(mx[2])};
    XYZICloud cropped;
    const auto t_crop = PhaseClock::clock::now();
    for (size_t i = 0; i < original.size(); ++i) {
      const float p[3] = {original.x[i], original.y[i], original.z[i]};
      if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
      bool in = true;
      for (int a = 0; a < 3; ++a) in = in && !(p[a] < fmn[a]) && !(p[a] > fmx[a]);
      if (in) cropped.push_back(p[0], p[1], p[2], original.intensity[i]);
    }
    std::cout << "Loaded point cloud with " << original.size() << " points." << std::endl;
    std::cout << "Cropped point cloud with " << cropped.size() << " points." << std::endl;
    const std::string cropPath = opt.outputPath + "scans-crop.pcd";  // outputPath must end in '/' (:131)
    if (opt.device_writer)
      deviceWriteXYZI(cropPath, cropped.x.data(), cropped.y.data(), cropped.z.data(), cropped.intensity.data(), cropped.size());
    else
      writeASCII_XYZI(cropPath, cropped.x.data(), cropped.y.data(), cropped.z.data(), cropped.intensity.data(), cropped.size());
    std::cout << "Cropped point cloud saved to: " << cropPath << std::endl;
    g_clock.add("crop_and_write_ascii_s", PhaseClock::since(t_crop));
    Phase ph_mls(opt.enableMLS ? "enable_mls_stage_s" : "cloud_move_s");
    if (opt.enableMLS) {
      // CloudSmooth re-reads the ASCII crop it was handed (cloudSmooth.cpp:92): 8 significant digits
      XYZICloud crop8;
      if (readPCD(cropPath, crop8) == -1) {
        std::cerr << "Couldn't read file " << cropPath << std::endl;
        return;
      }
      pcp_mls_params mp;
      pcp_default_mls_params(&mp);  // PointCloudProcessor.cpp:67-86
      if (opt.mls_voxel_size > 0.0f) mp.vgd_voxel_size = opt.mls_voxel_size;
      if (opt.mls_dilation_iterations >= 0) mp.vgd_iterations = opt.mls_dilation_iterations;
      if (opt.mls_upsampling >= 0) mp.upsampling = opt.mls_upsampling;
      if (opt.stream_colour) {
        // the chain runs later, chunk by chunk into the colour stage (streamedColourisation): `cloud` is its input here
        mls_params = mp;
        cloud = std::move(crop8);
        return;
      }
      if (opt.ortho_map) {  // (the frame is fitted to the map the run read, as the streamed form fits it)
        ortho_fit_xyz.resize(3 * crop8.size());
        for (size_t i = 0; i < crop8.size(); ++i) {
          ortho_fit_xyz[3 * i] = crop8.x[i];
          ortho_fit_xyz[3 * i + 1] = crop8.y[i];
          ortho_fit_xyz[3 * i + 2] = crop8.z[i];
        }
      }
      if (device_thread.joinable()) device_thread.join();  // (one thread at a time creates contexts: pcp_create sets process-wide defaults)
      MultiCloudSmooth smooth(opt.gpus);  // --gpus N: MLS queries / voxel chunks dealt out over the GPUs (pcp_multi.hpp)
      smooth.initialize(mp);
      smooth.setLocalPlaneSampling(opt.mls_upsampling_radius, opt.mls_upsampling_step);
      SmoothedCloud s = smooth.processWithOutlierRemoval(crop8.x.data(), crop8.y.data(), crop8.z.data(),
                                                         static_cast<int64_t>(crop8.size()));
      const std::string mlsPath = fs::path(cropPath).stem().string() + "_mls.pcd";  // CWD-relative, sic (B14)
      if (!opt.device_writer) {
        writeASCII_PointNormal(mlsPath, s.xyz.data(), s.normal.data(), s.curvature.data(), s.curvature.size());
      } else if (smooth.resultResident()) {  // the rows are still the smoothing context's result: formatted where they lie
        ChunkedAsciiWriter w(mlsPath, ChunkedAsciiWriter::PointNormal, static_cast<int64_t>(s.curvature.size()));
        for (int64_t first = 0;;) {
          const Device::TextWindow t = smooth.device(0).mlsFetchAscii(first, kTextWindowRows, text_);
          if (t.rows == 0) break;
          w.appendText(text_.data(), static_cast<size_t>(t.bytes), static_cast<size_t>(t.rows));
          first += t.rows;
        }
        (void)w.finish();
      } else {  // (the streamed fallback gathered its chunks on the host)
        std::vector<float> f(7 * s.curvature.size());
        for (size_t i = 0; i < s.curvature.size(); ++i) {
          for (size_t c = 0; c < 3; ++c) {
            f[7 * i + c] = s.xyz[3 * i + c];
            f[7 * i + 3 + c] = s.normal[3 * i + c];
          }
          f[7 * i + 6] = s.curvature[i];
        }
        (void)deviceWriteRows(smooth.device(0), mlsPath, ChunkedAsciiWriter::PointNormal, PCP_ROWS_POINTNORMAL, s.curvature.size(), f.data(),
                              nullptr, nullptr);
      }
      cloud.resize(s.curvature.size());
      for (size_t i = 0; i < cloud.size(); ++i) {
        cloud.x[i] = s.xyz[3 * i];
        cloud.y[i] = s.xyz[3 * i + 1];
        cloud.z[i] = s.xyz[3 * i + 2];
        cloud.intensity[i] = 0.0f;  // PointNormal carries no intensity (copyPointCloud, :144)
      }
      if (const char *dump = std::getenv("PCP_CLI_DUMP_SMOOTHED")) {
        // test hook: the smoothed cloud as the colour stage receives it (raw fp32 xyz triples; the ASCII file above
        // carries 8 significant digits, one short of a float's round trip)
        std::ofstream df(dump, std::ios::binary);
        df.write(reinterpret_cast<const char *>(s.xyz.data()), static_cast<std::streamsize>(s.xyz.size() * sizeof(float)));
      }
    } else {
      cloud = std::move(original);  // the reference reloads the same file (:148)
      std::cout << "Loaded point cloud with " << cloud.size() << " points." << std::endl;
    }
  }

  // ---- --deviceReader 1 ----------------------------------------------------------------------------------------------------
  // loadPCDFile, with the rows of an ASCII file parsed on the first device when --deviceReader 1 asks for it; whatever the device
  // reader does not take goes to the host reader whole, so the return value and the cloud are loadPCDFile's on every file
  int readPCD(const std::string &path, XYZICloud &into) {
    if (opt.device_reader) {
      const DeviceReadResult r = loadPCDFileDevice(path, [this]() -> Device & { return writerDevice(); }, into);
      if (r.loaded) return 0;
      if (!r.why.empty()) std::cerr << "--deviceReader 1: " << path << ": " << r.why << "; read by the host reader" << std::endl;
    }
    return loadPCDFile(path, into);
  }

  // ---- --deviceWriter 1 ----------------------------------------------------------------------------------------------------
  std::vector<char> text_;  // one window of text, reused by every site

  // the colour context, wherever in process() it is first needed (the crop is written before setupDevice)
  Device &writerDevice() {
    if (device_thread.joinable()) device_thread.join();
    if (device_error) std::rethrow_exception(device_error);
    if (!gpu) gpu.reset(new MultiDevice(opt.gpus));
    return gpu->device(0);
  }
  // a writeASCII_* site whose rows are host arrays (f row-major): header, then the rows formatted by pcp_ascii_rows window by
  // window.  0 / -1 and the empty-cloud exception as the host writers.
  int deviceWriteRows(Device &dev, const std::string &path, ChunkedAsciiWriter::Kind kind, int32_t rows_kind, size_t n, const float *f,
                      const uint8_t *rgb, const uint16_t *mask) {
    if (n == 0) throw std::runtime_error(detail::empty_cloud_message());
    {
      std::ofstream probe(path, std::ios::binary);  // (the host writers return -1 for a path that cannot be opened)
      if (!probe) return -1;
    }
    const size_t nf = rows_kind == PCP_ROWS_XYZI ? 4 : rows_kind == PCP_ROWS_POINTNORMAL ? 7 : 3;
    ChunkedAsciiWriter w(path, kind, static_cast<int64_t>(n));
    for (size_t first = 0; first < n; first += static_cast<size_t>(kTextWindowRows)) {
      const size_t rows = std::min(n - first, static_cast<size_t>(kTextWindowRows));
      const int64_t bytes = dev.asciiRows(rows_kind, static_cast<int64_t>(rows), f + nf * first, rgb ? rgb + 3 * first : nullptr,
                                          mask ? mask + first : nullptr, text_);
      w.appendText(text_.data(), static_cast<size_t>(bytes), rows);
    }
    return w.finish();
  }
  int deviceWriteXYZI(const std::string &path, const float *x, const float *y, const float *z, const float *intensity, size_t n) {
    std::vector<float> f(4 * n);
    for (size_t i = 0; i < n; ++i) {
      f[4 * i] = x[i];
      f[4 * i + 1] = y[i];
      f[4 * i + 2] = z[i];
      f[4 * i + 3] = intensity[i];
    }
    return deviceWriteRows(writerDevice(), path, ChunkedAsciiWriter::XYZI, PCP_ROWS_XYZI, n, f.data(), nullptr, nullptr);
  }
  // a final file from the colour result resident on the device: removePointsWithNoColor's `rows` survivors
  int deviceWriteColoured(const std::string &path, bool with_label, int64_t rows) {
    if (rows == 0) throw std::runtime_error(detail::empty_cloud_message());
    {
      std::ofstream probe(path, std::ios::binary);
      if (!probe) return -1;
    }
    ChunkedAsciiWriter w(path, with_label ? ChunkedAsciiWriter::XYZRGBMask : ChunkedAsciiWriter::XYZRGB, rows);
    for (int64_t first = 0;;) {
      const Device::TextWindow t = gpu->device(0).colourCompactAscii(with_label, first, kTextWindowRows, text_);
      if (t.rows == 0) break;
      w.appendText(text_.data(), static_cast<size_t>(t.bytes), static_cast<size_t>(t.rows));
      first += t.rows;
    }
    return w.finish();
  }

  void generateResultStorageFolder() {  // :1034-1048
    const fs::path dir(opt.outputPath + "filtered_pcd/");
    if (fs::exists(dir)) fs::remove_all(dir);
    fs::create_directories(dir);
  }

  void selectKeyframes() {  // :1050-1075 + markKeyframe hpp:151-191 (distance rule only, B9)
    keyframes.clear();
    int last_idx = -1;
    for (size_t i = 0; i < frames.size(); ++i) {
      bool key = last_idx < 0;
      if (key) std::cout << "First frame is always a keyframe." << std::endl;
      if (!key) {
        const auto &a = frames[i].pose, &b = frames[static_cast<size_t>(last_idx)].pose;
        const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
        key = std::sqrt(dx * dx + dy * dy + dz * dz) >= 0.1;
      }
      if (key) {
        keyframes.push_back(frames[i]);
        last_idx = static_cast<int>(i);
      }
    }
  }

  void setupDevice() {
    Phase ph("device_setup_and_cloud_upload_s");
    if (device_thread.joinable()) device_thread.join();
    if (device_error) std::rethrow_exception(device_error);
    if (!gpu) gpu.reset(new MultiDevice(opt.gpus));
    // (--streamColour 1: the colour context starts with an empty cloud, the chunks arrive from the smoothing context)
    gpu->uploadCloud(cloud.x.data(), cloud.y.data(), cloud.z.data(), opt.stream_colour ? 0 : static_cast<int64_t>(cloud.size()));
    // image size from the first keyframe image; cull size stays the reference's {4096,3000} (:206,:525)
    if (!keyframes.empty() && decoders) {  // (the decoders are on it already)
      std::unique_lock<std::mutex> lk(decoders->mu);
      decoders->cv.wait(lk, [&] { return decoders->ready[0] != 0; });
      const bool jpg = !decoders->jpg[0].empty();
      if (!jpg && decoders->img[0].empty()) throw std::runtime_error("Failed to read image from: " + keyframes[0].imagePath);
      img_w = jpg ? decoders->jpg[0].width : decoders->img[0].width;
      img_h = jpg ? decoders->jpg[0].height : decoders->img[0].height;
    } else if (!keyframes.empty()) {
      const Image8 first = read_image_bgr(keyframes[0].imagePath);
      if (first.empty()) throw std::runtime_error("Failed to read image from: " + keyframes[0].imagePath);
      img_w = first.width;
      img_h = first.height;
    }
    pcp_camera cam;
    pcp_default_camera(&cam);
    if (!keyframes.empty()) {
      cam.image_width = img_w;
      cam.image_height = img_h;
    }
    pcp_cull_params cull;
    pcp_default_cull_params(&cull);
    cull.cull_mode = opt.cull_mode;
    cull.match_mode = opt.match_mode;
    gpu->setCamera(cam, &cull);
    std::vector<pcp_pose> poses;
    for (const auto &k : keyframes) poses.push_back(k.pose);
    gpu->setKeyframes(poses);
    if (gpu->size() == 1 && opt.match_mode != PCP_MATCH_RADIUS && !opt.stream_colour) {  // (no chunk sees the whole cloud)
      // the reference credits a sample to EVERY map point within 10 um of it (radiusSearch, :571); --matchBack roundtrip to
      // the sample's own point.  Say so when the map holds points that close together (duplicates of merged scans).
      int64_t close = 0;
      if (pcp_close_pairs(gpu->device(0).get(), 2.5e-5, &close) != PCP_OK)  // a map with NaN / infinite points: no grid
        std::cerr << "Warning: " << pcp_last_error(gpu->device(0).get()) << "; the close-pair check is skipped." << std::endl;
      if (close > 0)
        std::cerr << "Warning: " << close << " map points have another point within 25 um; the reference would let them "
                  << "share colour samples (PointCloudProcessor.cpp:571), this build does not." << std::endl;
    }
  }

  void applyNIDBasedPoseOptimization() {  // :156-164 -> calibrate.cpp:42-126
    double cost = 0.0;
    // one GPU: VisualLiDARCalibration on the context; several: the keyframes' joint histograms are summed over the point
    // shards (MultiDevice::calibrate), no GPU ever holds the whole map
    gpu->uploadIntensity(cloud.intensity.data(), static_cast<int64_t>(cloud.size()));
    uploadImages(false);  // VisualLiDARCalibration reads the images itself, without generateColorMap's adjustment
    T_camera_lidar_optimized = gpu->calibrate(&cost);
    std::printf("Final cost: %.3f\n--- T_camera_lidar ---\n", cost);
    for (int r = 0; r < 4; ++r)
      std::printf("%g %g %g %g\n", T_camera_lidar_optimized[4 * r], T_camera_lidar_optimized[4 * r + 1],
                  T_camera_lidar_optimized[4 * r + 2], T_camera_lidar_optimized[4 * r + 3]);
    {  // full-precision copy of the result next to the outputs (not written by the reference)
      std::ofstream tf(opt.outputPath + "T_camera_lidar_optimized.txt");
      char buf[64];
      for (int k = 0; k < 16; ++k) {
        std::snprintf(buf, sizeof(buf), "%.17g%c", T_camera_lidar_optimized[static_cast<size_t>(k)], (k % 4 == 3) ? '\n' : ' ');
        tf << buf;
      }
    }
    std::vector<pcp_pose> poses;
    for (const auto &k : keyframes) poses.push_back(k.pose);
    gpu->setKeyframes(poses, T_camera_lidar_optimized.data(), 0);  // the enableNIDOptimize branch, :504-509
    images_uploaded = false;                                        // set_frames drops the images
  }

  void viewCullingAndSaveFilteredPcds() {  // :178-224
    const size_t n = cloud.size();
    std::vector<float> cam(3 * n);
    for (size_t k = 0; k < keyframes.size(); ++k) {
      const auto t_gpu = PhaseClock::clock::now();
      const std::vector<int32_t> kept = gpu->cull(static_cast<int>(k));
      gpu->cameraCoordinates(static_cast<int>(k), cam);
      g_clock.add("filtered_dumps_gpu_s", PhaseClock::since(t_gpu));
      Phase ph("filtered_dumps_write_ascii_s");
      std::vector<float> x(kept.size()), y(kept.size()), z(kept.size()), in(kept.size());
      for (size_t q = 0; q < kept.size(); ++q) {
        const size_t i = static_cast<size_t>(kept[q]);
        x[q] = cam[i];
        y[q] = cam[n + i];
        z[q] = cam[2 * n + i];
        in[q] = cloud.intensity[i];
      }
      const std::string path =
          opt.outputPath + "filtered_pcd/" + std::to_string(keyframes[k].imageTimestamp) + "_beforeNID" + ".pcd";
      if ((opt.device_writer ? deviceWriteXYZI(path, x.data(), y.data(), z.data(), in.data(), kept.size())
                             : writeASCII_XYZI(path, x.data(), y.data(), z.data(), in.data(), kept.size())) == -1)
        throw std::runtime_error("Couldn't save filtered point cloud to PCD file.");
      std::cout << "Before NID optimization: view culling pcd saved to: " << path << ", the point size is "
                << kept.size() << std::endl;
    }
  }

  // cv::imread of every keyframe (and mask) on all host cores -- the decoders are pure functions of the file -- while
  // this thread uploads them in keyframe order; at most `window` decoded keyframes are held at a time (a 4096x3000
  // frame is 37 MB).  The reference decodes one image per keyframe iteration on its one thread.  The decoders may be started
  // ahead of their consumer (startDecoders: process() does, while the device comes up): uploadImages then finds them running.
  struct Decoders {
    std::vector<Image8> img, gray;
    std::vector<JpegCoeffs> jpg;  // keyframes left to the device: img[k] stays empty
    std::vector<uint8_t> ready;
    std::mutex mu;
    std::condition_variable cv;
    size_t n = 0, next = 0, uploaded = 0, window = 0;
    bool stop = false;
    std::vector<std::thread> pool;
  };
  std::unique_ptr<Decoders> decoders;
  std::vector<uint8_t> path_counted;  // keyframes already counted in images_jpeg_on_device / images_decoded_on_host

  void startDecoders() {
    if (decoders) return;
    decoders.reset(new Decoders);
    Decoders &D = *decoders;
    D.n = keyframes.size();
    unsigned threads = std::max(1u, std::min(std::thread::hardware_concurrency(), 16u));
    if (const char *e = std::getenv("PCP_DECODE_THREADS")) threads = static_cast<unsigned>(std::max(1, std::atoi(e)));
    threads = static_cast<unsigned>(std::min<size_t>(threads, std::max<size_t>(D.n, 1)));
    D.window = 2 * static_cast<size_t>(threads) + 2;
    D.img.resize(D.n);
    D.jpg.resize(D.n);
    D.gray.resize(D.n);
    D.ready.assign(D.n, 0);
    auto worker = [this]() {
      Decoders &W = *decoders;
      for (;;) {
        size_t k;
        {
          std::unique_lock<std::mutex> lk(W.mu);
          W.cv.wait(lk, [&] { return W.stop || W.next >= W.n || W.next < W.uploaded + W.window; });
          if (W.stop || W.next >= W.n) return;
          k = W.next++;
        }
        const auto t_dec = PhaseClock::clock::now();
        // cv::imread, :716: a supported JPEG is entropy-decoded here and reconstructed on the device, anything else decoded here
        JpegCoeffs co = read_jpeg_coefficients(keyframes[k].imagePath);
        Image8 a;
        if (co.empty()) a = read_image_bgr(keyframes[k].imagePath);
        Image8 b;
        if (enableMaskSegmentation) b = read_image_gray(keyframes[k].maskImagePath);  // cv::IMREAD_GRAYSCALE, :775
        g_clock.add("images_decode_thread_seconds", PhaseClock::since(t_dec));  // summed over the decoder threads
        {
          std::lock_guard<std::mutex> lk(W.mu);
          W.img[k] = std::move(a);
          W.jpg[k] = std::move(co);
          W.gray[k] = std::move(b);
          W.ready[k] = 1;
        }
        W.cv.notify_all();
      }
    };
    for (unsigned t = 0; t < threads; ++t) D.pool.emplace_back(worker);
  }

  void stopDecoders() {
    if (!decoders) return;
    {
      std::lock_guard<std::mutex> lk(decoders->mu);
      decoders->stop = true;
    }
    decoders->cv.notify_all();
    for (auto &th : decoders->pool) th.join();
    decoders.reset();
  }

  void uploadImages(bool adjusted) {
    if (images_uploaded && images_adjusted == adjusted) {
      stopDecoders();
      return;
    }
    Phase ph_all("images_decode_and_upload_wall_s");  // decoders on the host threads, uploads on this one, overlapped
    gpu->setImageAdjust(adjusted);  // cvtColor(BGR2HSV) ... cvtColor(HSV2BGR), :722-741, fused into the upload
    if (opt.balance_images) {  // scripts/image_color_balance_autonomous.py over the keyframe folder, on the texels instead
      pcp_balance_params bp;
      pcp_default_balance_params(&bp);
      bp.tiles_x = opt.clahe_tiles_x;
      bp.tiles_y = opt.clahe_tiles_y;
      bp.clip_limit = opt.clahe_clip;
      bp.gamma = opt.balance_gamma;
      gpu->setImageBalance(&bp);
    }
    const size_t n = keyframes.size();
    mask_missing.assign(n, 0);
    startDecoders();  // (running already when process() started them ahead)
    Decoders &D = *decoders;
    g_clock.add("images_jpeg_on_device", 0.0);  // keyframes reconstructed on the device / decoded on the host, each counted
    g_clock.add("images_decoded_on_host", 0.0);  // once (the NID stage uploads them a second time)
    path_counted.resize(n, 0);
    try {
      for (size_t k = 0; k < n; ++k) {
        {
          std::unique_lock<std::mutex> lk(D.mu);
          D.cv.wait(lk, [&] { return D.ready[k] != 0; });
        }
        std::cout << "Reading image from: " << keyframes[k].imagePath << std::endl;
        const bool on_device = !D.jpg[k].empty();
        if (on_device ? (D.jpg[k].width != img_w || D.jpg[k].height != img_h)
                      : (D.img[k].empty() || D.img[k].width != img_w || D.img[k].height != img_h))
          throw std::runtime_error("Failed to read image from: " + keyframes[k].imagePath);
        {
          Phase ph_up("images_upload_calls_s");
          if (on_device)
            gpu->uploadImageJpeg(static_cast<int>(k), D.jpg[k]);
          else
            gpu->uploadImage(static_cast<int>(k), D.img[k].data.data(), static_cast<int64_t>(D.img[k].width) * 3);
        }
        if (!path_counted[k]) {
          path_counted[k] = 1;
          g_clock.add(on_device ? "images_jpeg_on_device" : "images_decoded_on_host", 1.0);
        }
        if (enableMaskSegmentation) {
          std::cout << "Reading segment mask image from: " << keyframes[k].maskImagePath << std::endl;
          if (!D.gray[k].empty() && D.gray[k].width == img_w && D.gray[k].height == img_h)
            gpu->uploadMask(static_cast<int>(k), D.gray[k].data.data(), D.gray[k].width);
          else
            mask_missing[k] = 1;  // generateSegmentMap logs it and returns an empty cloud, :776-781
        }
        {
          std::lock_guard<std::mutex> lk(D.mu);
          D.img[k] = Image8();
          D.jpg[k] = JpegCoeffs();
          D.gray[k] = Image8();
          D.uploaded = k + 1;
        }
        D.cv.notify_all();
      }
    } catch (...) {
      stopDecoders();
      throw;
    }
    stopDecoders();
    images_uploaded = true;
    images_adjusted = adjusted;
  }

  // --streamColour 1: CloudSmooth::process (:139-145) and pcdColorizationAndSmooth (:474-602) chunk by chunk.  The files are
  // those of the one-shot path: <stem>_mls.pcd (its row count is known when the stream begins), cloudInWorldWithRGB.pcd and,
  // with --fuseMasks 1, cloudInWorldWithRGBandMask.pcd (bodies to temporaries beside the outputs, headers once the counts are
  // known).
  void streamedColourisation() {
    uploadImages(true);
    if (opt.crack_maps) writeCrackMaps();
    if (opt.fuse_masks) {
      for (size_t k = 0; k < keyframes.size(); ++k)
        if (mask_missing[k]) throw std::runtime_error("Failed to read image from: " + keyframes[k].maskImagePath);
      gpu->setLabelFusion(true);
    }
    Phase ph("stream_colour_s");
    Device smoothing(0);
    smoothing.uploadCloud(cloud.x.data(), cloud.y.data(), cloud.z.data(), static_cast<int64_t>(cloud.size()));
    CloudSmooth cs(smoothing, mls_params);
    cs.setLocalPlaneSampling(opt.mls_upsampling_radius, opt.mls_upsampling_step);
    if (opt.ortho_map) {  // every chunk is added to the map as it is coloured
      gpu->device(0).orthoBegin(orthoFrame());
      cs.setOrthoAccumulate(true);
    }
    const std::string cropPath = opt.outputPath + "scans-crop.pcd";
    const std::string mlsPath = fs::path(cropPath).stem().string() + "_mls.pcd";  // CWD-relative, sic (B14)
    const std::string rgbPath = opt.outputPath + "cloudInWorldWithRGB.pcd", maskPath = opt.outputPath + "cloudInWorldWithRGBandMask.pcd";
    std::unique_ptr<ChunkedAsciiWriter> mls, mask, rgb;
    const bool full = !opt.skip_full_cloud;  // (--skip_full_cloud 1: the chunks' rows stay on the device, only the voxel rows leave it)
    if (full) rgb.reset(new ChunkedAsciiWriter(rgbPath, ChunkedAsciiWriter::XYZRGB));
    if (full && opt.fuse_masks) mask.reset(new ChunkedAsciiWriter(maskPath, ChunkedAsciiWriter::XYZRGBMask));
    const StreamedColourStats st = opt.device_writer ? cs.processAndColorizeStreamedText(
        gpu->device(0), opt.stream_chunk,
        [&](const TextRows &t) {
          if (!t.labelled) rgb->appendText(t.text, t.bytes, t.rows);
          else if (mask) mask->appendText(t.text, t.bytes, t.rows);
        },
        [&](const TextRows &t, int64_t kept_rows) {
          if (!mls) mls.reset(new ChunkedAsciiWriter(mlsPath, ChunkedAsciiWriter::PointNormal, kept_rows));
          mls->appendText(t.text, t.bytes, t.rows);
        },
        opt.fuse_masks, kTextWindowRows, opt.output_leaf, full) : cs.processAndColorizeStreamed(
        gpu->device(0), opt.stream_chunk,
        [&](const ColouredChunk &c) {
          rgb->appendColoured(c.xyz.data(), c.rgb.data(), nullptr, c.index.size());
          if (mask) mask->appendColoured(c.xyz.data(), c.rgb.data(), c.label.data(), c.index.size());
        },
        [&](const SmoothedCloud &s, int64_t kept_rows) {
          if (!mls) mls.reset(new ChunkedAsciiWriter(mlsPath, ChunkedAsciiWriter::PointNormal, kept_rows));
          mls->appendPointNormal(s.xyz.data(), s.normal.data(), s.curvature.data(), s.curvature.size());
        },
        opt.fuse_masks, opt.output_leaf, full);
    std::cout << "streamed colour: " << st.chunks << " chunks, " << st.rows << " rows, " << st.coloured << " coloured" << std::endl;
    g_clock.add("stream_colour_sweep_a_s", st.sweep_a_s);
    g_clock.add("stream_colour_sweep_b_s", st.sweep_b_s);
    if (opt.output_leaf > 0.0f) {
      g_clock.add("voxel_reduce_add_s", st.voxel_add_s);
      g_clock.add("voxel_reduce_finish_s", st.voxel_finish_s);
    }
    if (opt.ortho_map) {
      g_clock.add("ortho_add_s", st.ortho_add_s);
      writeOrthoFiles();
    }
    if (!mls) mls.reset(new ChunkedAsciiWriter(mlsPath, ChunkedAsciiWriter::PointNormal, 0));  // no row: the writer's exception
    if (mls->finish() == -1) throw std::runtime_error("Couldn't save the smoothed point cloud.");
    if (mask && mask->rows() > 0) {  // saveColorizedPointCloud(rgbCloud, withMask), :933-960
      if (mask->finish() == -1) throw std::runtime_error("Couldn't save colorized and segment colored point cloud.");
      std::cout << "All colored and segment colored cloud saved to: " << maskPath << std::endl;
    }
    if (rgb && rgb->rows() > 0) {  // :912-929
      if (rgb->finish() == -1) throw std::runtime_error("Couldn't save colorized point cloud.");
      std::cout << "All colored cloud saved to: " << rgbPath << std::endl;
    }
    if (opt.output_leaf > 0.0f) writeVoxelFiles();  // (the accumulation was finished after sweep B)
  }

  // --outputLeaf L: the finished voxel accumulation of the colour context as <out>cloudInWorldWithRGB_voxel.pcd and, with
  // --fuseMasks 1, <out>cloudInWorldWithRGBandMask_voxel.pcd, through the host writer (the files are small); then dropped
  void writeVoxelFiles() {
    Phase ph("voxel_pcd_write_ascii_s");
    Device &dev = gpu->device(0);
    const VoxelCloud v = dev.voxelReduceFetch(opt.fuse_masks);
    dev.voxelReduceEnd();
    const size_t m = v.count.size();
    std::cout << "voxel output: leaf " << opt.output_leaf << ", " << m << " voxels" << std::endl;
    if (m == 0) return;  // (no coloured row: no file, as the full-resolution files)
    if (opt.fuse_masks) {
      std::vector<uint16_t> mask(v.label.begin(), v.label.end());
      const std::string path = opt.outputPath + "cloudInWorldWithRGBandMask_voxel.pcd";
      if (writeASCII_XYZRGBMask(path, v.xyz.data(), v.rgb.data(), mask.data(), m) == -1)
        throw std::runtime_error("Couldn't save the voxel-grid colorized and segment colored point cloud.");
      std::cout << "Voxel-grid colored and segment colored cloud saved to: " << path << std::endl;
    }
    std::vector<float> x(m), y(m), z(m);
    for (size_t i = 0; i < m; ++i) {
      x[i] = v.xyz[3 * i];
      y[i] = v.xyz[3 * i + 1];
      z[i] = v.xyz[3 * i + 2];
    }
    const std::string path = opt.outputPath + "cloudInWorldWithRGB_voxel.pcd";
    if (writeASCII_XYZRGB(path, x.data(), y.data(), z.data(), v.rgb.data(), m) == -1)
      throw std::runtime_error("Couldn't save the voxel-grid colorized point cloud.");
    std::cout << "Voxel-grid colored cloud saved to: " << path << std::endl;
  }
  // the one-shot path: the colour result that was just made (and smoothed), reduced where it lies
  void reduceToVoxels() {
    {
      Phase ph("voxel_reduce_gpu_s");
      Device &dev = gpu->device(0);
      dev.voxelReduceBegin(opt.output_leaf);
      (void)dev.voxelReduceAdd();
      (void)dev.voxelReduceFinish();
    }
    writeVoxelFiles();
  }

  // one array as a NumPy format 1.0 file: little-endian, C order, the header padded to a multiple of 64 bytes
  static void writeNpyHead(std::ofstream &f, const char *descr, const std::vector<size_t> &shape) {
    std::string dict = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (";
    for (size_t k = 0; k < shape.size(); ++k) dict += std::to_string(shape[k]) + (shape.size() == 1 || k + 1 < shape.size() ? ", " : "");
    dict += "), }";
    while ((10 + dict.size() + 1) % 64 != 0) dict += ' ';
    dict += '\n';
    const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, static_cast<unsigned char>(dict.size() & 0xff),
                                    static_cast<unsigned char>(dict.size() >> 8)};
    f.write(reinterpret_cast<const char *>(head), sizeof(head));
    f.write(dict.data(), static_cast<std::streamsize>(dict.size()));
  }
  static void writeNpy(const std::string &path, const char *descr, const std::vector<size_t> &shape, const void *data, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    writeNpyHead(f, descr, shape);
    f.write(static_cast<const char *>(data), static_cast<std::streamsize>(bytes));
    f.close();
    if (!f) throw std::runtime_error("Couldn't save geometry map to: " + path);
  }

  // --geometryMaps 1: what scripts/genNormAndDistanceMask.py makes of filtered_pcd/ (generate_norm_masks :200-231,
  // generate_distance_masks :233-266), per selected keyframe, from the map on the device
  void writeGeometryMaps() {
    Device &dev = gpu->device(0);
    const bool normals = opt.normal_radius > 0.0f;
    if (normals) {
      Phase ph("normals_gpu_s");
      const int64_t valid = dev.estimateNormals(opt.normal_radius);
      std::cout << "map normals: radius " << opt.normal_radius << ", " << valid << " of " << cloud.size() << " points valid" << std::endl;
    }
    const fs::path dir(opt.outputPath + "geometry_maps/");
    if (fs::exists(dir)) fs::remove_all(dir);
    fs::create_directories(dir);
    const ViewCulling vc(dev);
    const size_t w = static_cast<size_t>(img_w), h = static_cast<size_t>(img_h);
    for (size_t k = 0; k < keyframes.size(); ++k) {
      GeometryMaps g;
      {
        Phase ph("geometry_maps_gpu_s");
        g = vc.geometryMaps(static_cast<int>(k), img_w, img_h, normals);
      }
      Phase ph_w("geometry_maps_write_s");
      const std::string stem = opt.outputPath + "geometry_maps/" + std::to_string(keyframes[k].imageTimestamp);
      writeNpy(stem + "_range.npy", "<f4", {h, w}, g.range.data(), g.range.size() * 4);
      writeNpy(stem + "_xyz.npy", "<f4", {h, w, 3}, g.xyz_cam.data(), g.xyz_cam.size() * 4);
      if (normals) writeNpy(stem + "_normal.npy", "<f4", {h, w, 3}, g.normal_cam.data(), g.normal_cam.size() * 4);
      writeNpy(stem + "_index.npy", "<i4", {h, w}, g.index.data(), g.index.size() * 4);
      std::cout << "Geometry maps saved to: " << stem << "_*.npy, " << g.pixels << " pixels occupied" << std::endl;
    }
  }

  // --crackMaps 1: what preprocess() of scripts/genNormAndDistanceMask.py (:150-198) gets from cv2.threshold :167 and
  // distance_transform_edt :168 per mask, from the masks on the device (uploadImages has run); runs of up to 8 keyframes
  // per call
  void writeCrackMaps() {
    Device &dev = gpu->device(0);
    const fs::path dir(opt.outputPath + "crack_maps/");
    if (fs::exists(dir)) fs::remove_all(dir);
    fs::create_directories(dir);
    const size_t w = static_cast<size_t>(img_w), h = static_cast<size_t>(img_h), px = w * h, n = keyframes.size();
    for (size_t k0 = 0; k0 < n;) {
      if (mask_missing[k0]) {
        std::cout << "Failed to read image from: " << keyframes[k0].maskImagePath << std::endl;
        ++k0;
        continue;
      }
      size_t k1 = k0 + 1;
      while (k1 < n && k1 < k0 + 8 && !mask_missing[k1]) ++k1;
      MaskDistance d;
      {
        Phase ph("crack_maps_gpu_s");
        d = dev.maskDistance(static_cast<int>(k0), static_cast<int>(k1 - k0), img_w, img_h, opt.crack_threshold);
      }
      Phase ph_w("crack_maps_write_s");
      for (size_t k = k0; k < k1; ++k) {
        const std::string stem = opt.outputPath + "crack_maps/" + std::to_string(keyframes[k].imageTimestamp);
        writeNpy(stem + "_edt2.npy", "<u4", {h, w}, d.d2.data() + (k - k0) * px, px * 4);
        writeNpy(stem + "_nearest.npy", "<i4", {h, w}, d.nearest.data() + (k - k0) * px, px * 4);
        std::cout << "Crack maps saved to: " << stem << "_edt2.npy, " << stem << "_nearest.npy" << std::endl;
      }
      k0 = k1;
    }
  }

  // --crackWidth 1: the second half of Crack.process() (compute_skeleton_edge_pts, scripts/genNormAndDistanceMask.py
  // :396-478) at every foreground pixel, per selected keyframe, from the masks and the raw map on the device (uploadImages has
  // run)
  void writeCrackWidth() {
    Device &dev = gpu->device(0);
    const fs::path dir(opt.outputPath + "crack_width/");
    if (fs::exists(dir)) fs::remove_all(dir);
    fs::create_directories(dir);
    const ViewCulling vc(dev);
    const size_t w = static_cast<size_t>(img_w), h = static_cast<size_t>(img_h);
    for (size_t k = 0; k < keyframes.size(); ++k) {
      if (mask_missing[k]) {
        std::cout << "Failed to read image from: " << keyframes[k].maskImagePath << std::endl;
        continue;
      }
      CrackWidth c;
      {
        Phase ph("crack_width_gpu_s");
        c = vc.crackWidth(static_cast<int>(k), img_w, img_h, opt.crack_threshold, opt.crack_plane_radius);
      }
      Phase ph_w("crack_width_write_s");
      const std::string stem = opt.outputPath + "crack_width/" + std::to_string(keyframes[k].imageTimestamp);
      writeNpy(stem + "_width.npy", "<f4", {h, w}, c.width_m.data(), c.width_m.size() * 4);
      writeNpy(stem + "_edges.npy", "<i4", {h, w, 4}, c.edges.data(), c.edges.size() * 4);
      writeNpy(stem + "_flags.npy", "|u1", {h, w}, c.flags.data(), c.flags.size());
      writeNpy(stem + "_points.npy", "<f4", {h, w, 6}, c.points.data(), c.points.size() * 4);
      std::cout << "Crack width maps saved to: " << stem << "_*.npy, " << c.sites << " sites, " << c.widths << " widths" << std::endl;
    }
  }

  // --crackFuse 1: the per-point records of compute_skeleton_edge_pts (scripts/genNormAndDistanceMask.py :396-478) and its
  // result file (:476-478) for the whole map: the widths of every keyframe brought back to the map points, and the cracks
  void writeCrackFuse() {
    Device &dev = gpu->device(0);
    const fs::path dir(opt.outputPath + "crack_width/");
    fs::create_directories(dir);  // (--crackWidth 1 has made and filled it)
    std::vector<int> added;
    for (size_t k = 0; k < keyframes.size(); ++k) {
      if (mask_missing[k])
        std::cout << "Failed to read image from: " << keyframes[k].maskImagePath << std::endl;
      else
        added.push_back(static_cast<int>(k));
    }
    CrackMap m;
    CrackLengths cl;
    CrackSkeleton sk;
    CrackDirections cdir;
    CrackBranches cbr;
    {
      const auto t0 = PhaseClock::clock::now();
      m = ViewCulling(dev).crackMap(added, static_cast<int64_t>(cloud.size()), opt.crack_threshold, opt.crack_plane_radius,
                                    opt.crack_min_views, opt.crack_link_radius, opt.crack_length ? &cl : nullptr,
                                    opt.crack_skeleton ? &sk : nullptr, opt.crack_skeleton_step, opt.crack_direction ? &cdir : nullptr,
                                    opt.crack_branches ? &cbr : nullptr, opt.crack_prune);
      g_clock.add("crack_fuse_gpu_s", PhaseClock::since(t0) - cl.seconds - sk.seconds - cdir.seconds - cbr.seconds);
      if (opt.crack_branches) g_clock.add("crack_branches_gpu_s", cbr.seconds);
      if (opt.crack_direction) g_clock.add("crack_direction_gpu_s", cdir.seconds);
      if (opt.crack_length) g_clock.add("crack_length_gpu_s", cl.seconds);
      if (opt.crack_skeleton) g_clock.add("crack_skeleton_gpu_s", sk.seconds);
    }
    Phase ph_w("crack_fuse_write_s");
    const size_t n = cloud.size();
    const std::string stem = opt.outputPath + "crack_width/";
    writeNpy(stem + "map_width.npy", "<f4", {n}, m.width_mean.data(), n * 4);
    writeNpy(stem + "map_width_best.npy", "<f4", {n}, m.width_best.data(), n * 4);
    writeNpy(stem + "map_views.npy", "<u4", {n}, m.views.data(), n * 4);
    writeNpy(stem + "map_crack.npy", "<i4", {n}, m.label.data(), n * 4);
    // --facets 1: the most frequent facet id among a crack's points, ties to the lowest id, -1 when none has one
    std::vector<int32_t> crack_facet(m.ids.size(), -1);
    if (opt.facets) {
      std::vector<std::map<int32_t, int64_t>> votes(m.ids.size());
      for (size_t i = 0; i < n; ++i) {
        if (m.label[i] < 0 || facets_.label[i] < 0) continue;
        const size_t r = static_cast<size_t>(std::lower_bound(m.ids.begin(), m.ids.end(), m.label[i]) - m.ids.begin());
        votes[r][facets_.label[i]] += 1;
      }
      for (size_t r = 0; r < votes.size(); ++r) {
        int64_t most = 0;
        for (const auto &kv : votes[r])  // (ascending ids: a tie keeps the lowest)
          if (kv.second > most) most = kv.second, crack_facet[r] = kv.first;
      }
    }
    std::ofstream f(stem + "cracks_3d.json");
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.9g", v);
      return std::string(b);
    };
    const double mm = 1000.0 / 1048576.0;  // quanta of 2^-20 m to millimetres
    f << "[";
    for (size_t r = 0; r < m.ids.size(); ++r) {
      const int64_t *st = m.stats.data() + 5 * r;
      const float *bx = m.box.data() + 6 * r;
      f << (r ? ",\n " : "\n ") << "{\"id\": " << m.ids[r] << ", \"points\": " << st[0] << ", \"centre_points\": " << st[4]
        << ", \"width_mean_mm\": " << num(static_cast<double>(st[1]) / static_cast<double>(st[0]) * mm)
        << ", \"width_min_mm\": " << num(static_cast<double>(st[2]) * mm) << ", \"width_max_mm\": " << num(static_cast<double>(st[3]) * mm)
        << ", \"box_min\": [" << num(bx[0]) << ", " << num(bx[1]) << ", " << num(bx[2]) << "], \"box_max\": [" << num(bx[3]) << ", "
        << num(bx[4]) << ", " << num(bx[5]) << "]";
      if (opt.facets) f << ", \"facet\": " << crack_facet[r];
      f << "}";
    }
    f << "\n]\n";
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the cracks of the map.");
    std::cout << "Crack widths on the map saved to: " << stem << "map_*.npy and cracks_3d.json, " << added.size() << " keyframes, " << m.credited
              << " credited samples, " << m.crack_points << " crack points, " << m.ids.size() << " cracks" << std::endl;
    if (opt.crack_length) writeCrackLengths(cl, stem);
    if (opt.crack_skeleton) writeCrackSkeleton(sk, m, stem);
    if (opt.crack_direction) writeCrackDirections(cdir, crack_facet, stem);
    if (opt.crack_branches) writeCrackBranches(cbr, m, crack_facet, stem);
    if (opt.ortho_map && !opt.ortho_by_facet) {  // the widths and the cracks drawn on the orthographic map: map_width[index], map_crack[index]
      const size_t h = static_cast<size_t>(ortho_frame_used.height), w = static_cast<size_t>(ortho_frame_used.width);
      std::vector<float> width(ortho_index.size(), 0.0f);
      std::vector<int32_t> crack(ortho_index.size(), -1);
      // (the index layer names rows of the map the crack chain ran on: --crackFuse 1 is refused with --enableMLS 1)
      for (size_t p = 0; p < ortho_index.size(); ++p) {
        if (ortho_index[p] == 0xFFFFFFFFu) continue;
        if (ortho_index[p] >= n)
          throw std::runtime_error("the orthographic map's index layer names row " + std::to_string(ortho_index[p]) + " of a map of " +
                                   std::to_string(n) + " points: the crack layers cannot be drawn");
        width[p] = m.width_mean[ortho_index[p]];
        crack[p] = m.label[ortho_index[p]];
      }
      writeNpy(opt.outputPath + "ortho/ortho_width.npy", "<f4", {h, w}, width.data(), width.size() * 4);
      writeNpy(opt.outputPath + "ortho/ortho_crack.npy", "<i4", {h, w}, crack.data(), crack.size() * 4);
      std::cout << "Orthographic crack layers saved to: " << opt.outputPath << "ortho/ortho_width.npy, ortho_crack.npy" << std::endl;
    }
  }

  // --compareMap base.pcd: the map against an earlier survey (DESIGN.md "Map comparison"): the map normals, turned towards the
  // mean keyframe position (kept as they are without keyframes), the comparison, the three arrays and compare.json
  void writeCompare() {
    Device &dev = gpu->device(0);
    XYZICloud base;
    {
      Phase ph("compare_read_s");
      if (readPCD(opt.compare_map, base) == -1) throw std::runtime_error("Couldn't read the base point cloud file: " + opt.compare_map);
    }
    std::vector<float> rows(3 * base.size());
    for (size_t j = 0; j < base.size(); ++j) {
      rows[3 * j] = base.x[j];
      rows[3 * j + 1] = base.y[j];
      rows[3 * j + 2] = base.z[j];
    }
    pcp_compare_params p = opt.compare;
    double viewer[3];
    if (meanKeyframePosition(viewer)) {
      p.orient_mode = 1;
      for (int a = 0; a < 3; ++a) p.orient[a] = static_cast<float>(viewer[a]);
    }
    {
      Phase ph("compare_gpu_s");
      const int64_t valid = dev.estimateNormals(opt.normal_radius);
      std::cout << "map normals: radius " << opt.normal_radius << ", " << valid << " of " << cloud.size() << " points valid" << std::endl;
      compare_ = dev.compareMap(p, rows.data(), static_cast<int64_t>(base.size()), opt.compare_register ? &opt.reg : nullptr, &registration_);
    }
    Phase ph_w("compare_write_s");
    const std::string stem = opt.outputPath + "compare/";
    fs::create_directories(fs::path(stem));
    const size_t n = cloud.size();
    writeNpy(stem + "distance.npy", "<f4", {n}, compare_.distance.data(), n * 4);
    writeNpy(stem + "lod.npy", "<f4", {n}, compare_.lod.data(), n * 4);
    writeNpy(stem + "status.npy", "|u1", {n}, compare_.status.data(), n);
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.9g", v);
      return std::string(b);
    };
    int64_t significant = 0;
    double sum = 0.0, lo = 0.0, hi = 0.0;
    for (size_t i = 0; i < n; ++i) {
      if (compare_.status[i] < 4) continue;
      const double d = compare_.distance[i];
      lo = significant ? std::min(lo, d) : d;
      hi = significant ? std::max(hi, d) : d;
      sum += d;
      ++significant;
    }
    std::ofstream f(stem + "compare.json");
    f << "{\"base\": " << base.size() << ", \"points\": " << n << ", \"radius\": " << num(p.cyl_radius) << ", \"half_length\": " << num(p.cyl_half_length)
      << ", \"reg_error\": " << num(p.reg_error) << ", \"min_points\": " << p.min_points << ", \"normal_radius\": " << num(opt.normal_radius)
      << ", \"orient_mode\": " << p.orient_mode << ", \"viewer\": [" << num(p.orient[0]) << ", " << num(p.orient[1]) << ", " << num(p.orient[2])
      << "], \"stats\": [";
    for (int k = 0; k < 8; ++k) f << (k ? ", " : "") << compare_.stats[k];
    f << "], \"core\": " << compare_.stats[0] << ", \"measured\": " << compare_.stats[1] << ", \"positive\": " << compare_.stats[2]
      << ", \"negative\": " << compare_.stats[3] << ", \"no_counterpart\": " << compare_.stats[4] << ", \"too_few_own\": " << compare_.stats[5]
      << ", \"most_candidates\": " << compare_.stats[6] << ", \"significant\": " << significant << ", \"significant_mean\": "
      << num(significant ? sum / static_cast<double>(significant) : 0.0) << ", \"significant_min\": " << num(lo) << ", \"significant_max\": " << num(hi)
      << "}\n";
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the comparison of the map.");
    if (opt.compare_register) writeRegistration(stem, base.size());
    std::cout << "Map comparison saved to: " << stem << "distance.npy, lod.npy, status.npy and compare.json, " << compare_.stats[1] << " of "
              << compare_.stats[0] << " core points measured, " << compare_.stats[2] << " significant positive, " << compare_.stats[3]
              << " negative, " << compare_.stats[4] << " without a counterpart" << std::endl;
  }

  // --compareRegister 1: what the registration found (DESIGN.md "Map registration", RG8), beside the comparison made after it
  void writeRegistration(const std::string &stem, size_t base_rows) {
    const Registration &r = registration_;
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.17g", v);
      return std::string(b);
    };
    std::ofstream t(stem + "base_transform.txt");
    for (int a = 0; a < 4; ++a) t << num(r.T[4 * a]) << " " << num(r.T[4 * a + 1]) << " " << num(r.T[4 * a + 2]) << " " << num(r.T[4 * a + 3]) << "\n";
    t.close();
    std::ofstream f(stem + "registration.json");
    f << "{\"base\": " << base_rows << ", \"match_radius\": " << num(opt.reg.match_radius) << ", \"max_plane_distance\": " << num(opt.reg.max_plane_distance)
      << ", \"sample_stride\": " << opt.reg.sample_stride << ", \"max_iterations\": " << opt.reg.max_iterations << ", \"min_pairs\": " << opt.reg.min_pairs
      << ", \"tolerance\": " << num(opt.reg.tolerance) << ", \"cond_tol\": " << num(opt.reg.cond_tol) << ", \"normal_radius\": " << num(opt.normal_radius)
      << ", \"T\": [";
    for (int a = 0; a < 4; ++a)
      f << (a ? ", " : "") << "[" << num(r.T[4 * a]) << ", " << num(r.T[4 * a + 1]) << ", " << num(r.T[4 * a + 2]) << ", " << num(r.T[4 * a + 3]) << "]";
    f << "], \"log\": [";
    for (int32_t k = 0; k < r.iterations; ++k) {
      const double *row = r.log.data() + 5 * static_cast<size_t>(k);
      f << (k ? ", " : "") << "[" << num(row[0]) << ", " << num(row[1]) << ", " << num(row[2]) << ", " << num(row[3]) << ", " << num(row[4]) << "]";
    }
    f << "], \"status\": " << r.status << ", \"iterations\": " << r.iterations << ", \"pairs\": " << r.pairs << ", \"dof\": " << r.dof
      << ", \"rms\": " << num(r.rms) << "}\n";
    f.close();
    if (!t || !f) throw std::runtime_error("Couldn't save the registration of the base.");
    static const char *const names[] = {"converged", "iteration limit", "too few pairs"};
    std::cout << "Base registration saved to: " << stem << "registration.json and base_transform.txt, " << names[r.status < 0 || r.status > 2 ? 1 : r.status]
              << " after " << r.iterations << " iterations, " << r.pairs << " pairs, " << r.dof << " of 6 components, rms " << r.rms
              << " m (a candidate for --compareRegError)" << std::endl;
  }

  // --facets 1: the faces of the structure (DESIGN.md "Planar facets"): the map normals, the partition, the planes from the integers
  void writeFacets() {
    Device &dev = gpu->device(0);
    {
      Phase ph("facets_gpu_s");
      const int64_t valid = dev.estimateNormals(opt.normal_radius);
      std::cout << "map normals: radius " << opt.normal_radius << ", " << valid << " of " << cloud.size() << " points valid" << std::endl;
      facets_ = dev.facets(opt.facet);
    }
    Phase ph_w("facets_write_s");
    facets_.planes([&](int32_t id, int a) { const size_t i = static_cast<size_t>(id); return a == 0 ? cloud.x[i] : a == 1 ? cloud.y[i] : cloud.z[i]; },
                   static_cast<double>(opt.facet_max_rms));
    const std::string stem = opt.outputPath + "facets/";
    fs::create_directories(fs::path(stem));
    writeNpy(stem + "facet_label.npy", "<i4", {cloud.size()}, facets_.label.data(), cloud.size() * 4);
    std::ofstream f(stem + "facets.json");
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.9g", v);
      return std::string(b);
    };
    size_t planar = 0, cylindrical = 0;
    // --facetCylinders 1: the cylinder of every facet that is not planar, from its points and their normals
    facet_cyl_.assign(opt.facet_cylinders ? facets_.ids.size() : 0, pcp_cyl_frame{});
    std::vector<pcp_cyl_frame> &cyl = facet_cyl_;  // (kept: writeOrthoMapsByFacet unrolls the cylindrical facets through these frames)
    std::vector<double> cyl_stats(8 * cyl.size(), 0.0);
    std::vector<uint8_t> fitted(cyl.size(), 0);
    if (opt.facet_cylinders) {
      const size_t n = cloud.size();
      map_normals_.assign(3 * n, 0.0f);
      if (pcp_normals_fetch(dev.get(), map_normals_.data(), nullptr, nullptr) != PCP_OK)
        throw std::runtime_error(std::string("pcp_hip: ") + pcp_last_error(dev.get()));
      const std::vector<float> xyz = interleavedMap();
      double viewer[3];
      const bool seen = meanKeyframePosition(viewer);
      std::vector<uint8_t> member(n);
      facet_kind_.assign(facets_.ids.size(), 0);
      for (size_t r = 0; r < facets_.ids.size(); ++r) {
        if (facets_.planar[r]) {
          facet_kind_[r] = 1;
          continue;
        }
        for (size_t i = 0; i < n; ++i) member[i] = facets_.label[i] == facets_.ids[r] ? 1 : 0;
        std::string why;
        fitted[r] = Device::orthoFitCylinder(static_cast<int64_t>(n), xyz.data(), map_normals_.data(), member.data(), seen ? viewer : nullptr,
                                             opt.ortho_gsd, &cyl[r], cyl_stats.data() + 8 * r, &why) ? 1 : 0;
        if (!fitted[r]) std::cout << "facet " << facets_.ids[r] << ": no cylinder (" << why << ")" << std::endl;
        if (fitted[r] && cyl_stats[8 * r + 1] <= static_cast<double>(opt.facet_max_rms)) facet_kind_[r] = 2, ++cylindrical;
      }
    }
    auto vec3 = [&](const float *v) { return "[" + num(v[0]) + ", " + num(v[1]) + ", " + num(v[2]) + "]"; };
    f << "[";
    for (size_t r = 0; r < facets_.ids.size(); ++r) {
      const double *pl = facets_.plane.data() + 7 * r;
      const float *bx = facets_.box.data() + 6 * r;
      planar += facets_.planar[r];
      f << (r ? ",\n " : "\n ") << "{\"id\": " << facets_.ids[r] << ", \"points\": " << facets_.rows[10 * r] << ", \"centroid\": [" << num(pl[0]) << ", "
        << num(pl[1]) << ", " << num(pl[2]) << "], \"normal\": [" << num(pl[3]) << ", " << num(pl[4]) << ", " << num(pl[5]) << "], \"rms\": "
        << num(pl[6]) << ", \"planar\": " << (facets_.planar[r] ? "true" : "false") << ", \"box_min\": [" << num(bx[0]) << ", " << num(bx[1]) << ", "
        << num(bx[2]) << "], \"box_max\": [" << num(bx[3]) << ", " << num(bx[4]) << ", " << num(bx[5]) << "]";
      if (opt.facet_cylinders) {
        f << ", \"kind\": " << static_cast<int>(facet_kind_[r]);
        if (fitted[r]) {
          const pcp_cyl_frame &c = cyl[r];
          const double *st = cyl_stats.data() + 8 * r;
          f << ", \"cylinder\": {\"c\": " << vec3(c.c) << ", \"a\": " << vec3(c.a) << ", \"e\": " << vec3(c.e) << ", \"b\": " << vec3(c.b)
            << ", \"radius\": " << num(c.radius) << ", \"gsd\": " << num(c.gsd) << ", \"width\": " << c.width << ", \"height\": " << c.height
            << ", \"d_min\": " << num(c.d_min) << ", \"d_max\": " << num(c.d_max) << ", \"side\": " << c.side
            << ", \"rows\": " << static_cast<long long>(st[0]) << ", \"rms\": " << num(st[1]) << ", \"dev_min\": " << num(st[2])
            << ", \"dev_max\": " << num(st[3]) << ", \"arc\": " << num(st[4]) << ", \"eigenvalues\": [" << num(st[5]) << ", " << num(st[6])
            << ", " << num(st[7]) << "]}";
        }
      }
      f << "}";
    }
    f << "\n]\n";
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the facets of the map.");
    if (opt.facet_cylinders) std::cout << "Cylindrical facets: " << cylindrical << " of " << facets_.ids.size() - planar << " that are not planar" << std::endl;
    std::cout << "Facets saved to: " << stem << "facet_label.npy and facets.json, " << facets_.facet_points << " facet points, " << facets_.components
              << " components, " << facets_.ids.size() << " facets, " << planar << " planar" << std::endl;
  }

  // --orthoMap 1 --orthoFrame facets: one map per planar facet, on a frame fitted to the facet's own points (seen from the mean
  // keyframe position) and drawn from those points only, into <out>ortho/facet_<row>/
  // the map the run read as interleaved rows, and the mean keyframe position (false: no keyframes)
  std::vector<float> interleavedMap() const {
    const size_t n = cloud.size();
    std::vector<float> xyz(3 * n);
    for (size_t i = 0; i < n; ++i) {
      xyz[3 * i] = cloud.x[i];
      xyz[3 * i + 1] = cloud.y[i];
      xyz[3 * i + 2] = cloud.z[i];
    }
    return xyz;
  }
  bool meanKeyframePosition(double viewer[3]) const {
    viewer[0] = viewer[1] = viewer[2] = 0.0;
    for (const Frame &k : keyframes) {
      viewer[0] += k.pose.x / static_cast<double>(keyframes.size());
      viewer[1] += k.pose.y / static_cast<double>(keyframes.size());
      viewer[2] += k.pose.z / static_cast<double>(keyframes.size());
    }
    return !keyframes.empty();
  }

  void writeOrthoMapsByFacet() {
    Device &dev = gpu->device(0);
    const size_t n = cloud.size();
    const std::vector<float> xyz = interleavedMap();
    double viewer[3];
    (void)meanKeyframePosition(viewer);
    std::vector<uint8_t> member(n);
    size_t maps = 0, unrolled = 0;
    for (size_t r = 0; r < facets_.ids.size(); ++r) {
      if (opt.facet_cylinders && facet_kind_[r] == 2) {  // the facet unrolled through its cylinder (DESIGN.md "Cylindrical facets")
        const int32_t id = facets_.ids[r];
        const pcp_cyl_frame &cf = facet_cyl_[r];  // (the frame facets.json records: fitted once, in writeFacets)
        {
          Phase ph("ortho_gpu_s");
          dev.orthoBeginCyl(cf);
          (void)dev.orthoAddFacet(id, 0);
        }
        if (opt.ortho_texture && !opt.ortho_texture_cylinders)
          std::cerr << "facet " << id << " (ortho/facet_" << r << "/): cylindrical, skipped by --orthoTexture (orthophotos of unrolled maps are not built)"
                    << std::endl;
        writeOrthoFiles(opt.outputPath + "ortho/facet_" + std::to_string(r) + "/", &cf);
        ++unrolled;
        continue;
      }
      if (!facets_.planar[r]) continue;
      const int32_t id = facets_.ids[r];
      {
        Phase ph("ortho_frame_s");
        for (size_t i = 0; i < n; ++i) member[i] = facets_.label[i] == id ? 1 : 0;
        ortho_frame_used = Device::orthoFitFrame(static_cast<int64_t>(n), xyz.data(), member.data(), keyframes.empty() ? nullptr : viewer, opt.ortho_gsd);
      }
      {
        Phase ph("ortho_gpu_s");
        dev.orthoBegin(ortho_frame_used);
        (void)dev.orthoAddFacet(id, 0);
      }
      writeOrthoFiles(opt.outputPath + "ortho/facet_" + std::to_string(r) + "/");
      ++maps;
    }
    std::cout << "Orthographic maps by facet: " << maps << " planar facets of " << facets_.ids.size() << std::endl;
    if (opt.facet_cylinders) std::cout << "Unrolled maps by facet: " << unrolled << " cylindrical facets of " << facets_.ids.size() << std::endl;
  }

  // --orthoMap 1: the frame.  auto: the plane fitted to the finite points of the map the run read, seen from the side of the
  // mean keyframe position.  Nine numbers: o, u, v as given, n = u x v, the raster sized to hold the map's points on the
  // positive side of the origin (one spare pixel: the library rounds in fp32), the depth window unbounded.
  pcp_ortho_frame orthoFrame() {
    Phase ph("ortho_frame_s");
    const bool own = !ortho_fit_xyz.empty();
    const size_t n = own ? ortho_fit_xyz.size() / 3 : cloud.size();
    auto at = [&](size_t i, int a) { return own ? ortho_fit_xyz[3 * i + static_cast<size_t>(a)] : (a == 0 ? cloud.x[i] : a == 1 ? cloud.y[i] : cloud.z[i]); };
    pcp_ortho_frame f{};
    if (opt.ortho_frame.empty()) {
      std::vector<float> xyz(3 * n);
      std::vector<uint8_t> finite(n);
      for (size_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) xyz[3 * i + static_cast<size_t>(a)] = at(i, a);
        finite[i] = std::isfinite(xyz[3 * i]) && std::isfinite(xyz[3 * i + 1]) && std::isfinite(xyz[3 * i + 2]) ? 1 : 0;
      }
      double viewer[3] = {0.0, 0.0, 0.0};
      for (const Frame &k : keyframes) {
        viewer[0] += k.pose.x / static_cast<double>(keyframes.size());
        viewer[1] += k.pose.y / static_cast<double>(keyframes.size());
        viewer[2] += k.pose.z / static_cast<double>(keyframes.size());
      }
      f = Device::orthoFitFrame(static_cast<int64_t>(n), xyz.data(), finite.data(), keyframes.empty() ? nullptr : viewer, opt.ortho_gsd);
    } else {
      const float *v = opt.ortho_frame.data();
      for (int a = 0; a < 3; ++a) {
        f.o[a] = v[a];
        f.u[a] = v[3 + a];
        f.v[a] = v[6 + a];
      }
      f.n[0] = f.u[1] * f.v[2] - f.u[2] * f.v[1];
      f.n[1] = f.u[2] * f.v[0] - f.u[0] * f.v[2];
      f.n[2] = f.u[0] * f.v[1] - f.u[1] * f.v[0];
      f.gsd = opt.ortho_gsd;
      f.d_min = -FLT_MAX;
      f.d_max = FLT_MAX;
      double smax = 0.0, tmax = 0.0;
      for (size_t i = 0; i < n; ++i) {
        const double d[3] = {at(i, 0) - static_cast<double>(f.o[0]), at(i, 1) - static_cast<double>(f.o[1]), at(i, 2) - static_cast<double>(f.o[2])};
        if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2])) continue;
        smax = std::max(smax, d[0] * f.u[0] + d[1] * f.u[1] + d[2] * f.u[2]);
        tmax = std::max(tmax, d[0] * f.v[0] + d[1] * f.v[1] + d[2] * f.v[2]);
      }
      f.width = static_cast<int32_t>(std::min(1e9, std::floor(smax / opt.ortho_gsd) + 2.0));
      f.height = static_cast<int32_t>(std::min(1e9, std::floor(tmax / opt.ortho_gsd) + 2.0));
    }
    ortho_frame_used = f;
    return f;
  }
  // the one-shot path: the colour result that was just made (and smoothed), drawn where it lies
  void writeOrthoMap() {
    {
      Phase ph("ortho_gpu_s");
      Device &dev = gpu->device(0);
      dev.orthoBegin(orthoFrame());
      (void)dev.orthoAdd(0);
    }
    writeOrthoFiles();
  }
  // the map begun on the colour context, finished with --orthoFill, as <out>ortho/ortho_*.npy and ortho_frame.json; then dropped
  // (cyl: the map was begun under this cylinder's frame -- ortho_frame.json holds the cylinder, and the orthophoto is made only
  // under --orthoTextureCylinders 1)
  void writeOrthoFiles(const std::string &stem_in = std::string(), const pcp_cyl_frame *cyl = nullptr) {
    const std::string stem = stem_in.empty() ? opt.outputPath + "ortho/" : stem_in;
    Device &dev = gpu->device(0);
    const bool photo = opt.ortho_texture && (!cyl || opt.ortho_texture_cylinders);
    OrthoMap m;
    {
      Phase ph("ortho_finish_gpu_s");
      m = dev.orthoFetch(opt.ortho_fill, opt.fuse_masks);
      if (!photo && !opt.ortho_defects) dev.orthoEnd();
    }
    if (opt.ortho_defects) {  // (on the finished map, before it ends)
      writeOrthoDefects(dev, m.frame, stem);
      if (!photo) dev.orthoEnd();
    }
    if (photo) {
      struct End {  // also on the way out of an exception
        Device &d;
        ~End() { (void)pcp_ortho_end(d.get()); }
      } end{dev};
      writeOrthoPhoto(dev, m.frame, stem, cyl != nullptr);
    }
    Phase ph_w("ortho_write_s");
    fs::create_directories(fs::path(stem));
    const size_t h = static_cast<size_t>(m.frame.height), w = static_cast<size_t>(m.frame.width);
    writeNpy(stem + "ortho_rgb.npy", "|u1", {h, w, 3}, m.rgb.data(), m.rgb.size());
    writeNpy(stem + "ortho_depth.npy", "<f4", {h, w}, m.depth.data(), m.depth.size() * 4);
    writeNpy(stem + "ortho_index.npy", "<u4", {h, w}, m.index.data(), m.index.size() * 4);
    writeNpy(stem + "ortho_status.npy", "|u1", {h, w}, m.status.data(), m.status.size());
    if (opt.fuse_masks) writeNpy(stem + "ortho_label.npy", "|u1", {h, w}, m.label.data(), m.label.size());
    std::ofstream f(stem + "ortho_frame.json");
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.9g", v);
      return std::string(b);
    };
    auto vec = [&](const float *v) { return "[" + num(v[0]) + ", " + num(v[1]) + ", " + num(v[2]) + "]"; };
    if (cyl)
      f << "{\"kind\": \"cylinder\", \"c\": " << vec(cyl->c) << ", \"a\": " << vec(cyl->a) << ", \"e\": " << vec(cyl->e) << ", \"b\": " << vec(cyl->b)
        << ", \"radius\": " << num(cyl->radius) << ", \"side\": " << cyl->side << ", \"gsd\": " << num(cyl->gsd) << ", \"width\": " << cyl->width
        << ", \"height\": " << cyl->height << ", \"d_min\": " << num(cyl->d_min) << ", \"d_max\": " << num(cyl->d_max)
        << ", \"fill_radius\": " << opt.ortho_fill << ", \"contributors\": " << m.contributors << ", \"occupied\": " << m.occupied
        << ", \"filled\": " << m.filled << "}\n";
    else
      f << "{\"o\": " << vec(m.frame.o) << ", \"u\": " << vec(m.frame.u) << ", \"v\": " << vec(m.frame.v) << ", \"n\": " << vec(m.frame.n)
        << ", \"gsd\": " << num(m.frame.gsd) << ", \"width\": " << m.frame.width << ", \"height\": " << m.frame.height
        << ", \"d_min\": " << num(m.frame.d_min) << ", \"d_max\": " << num(m.frame.d_max) << ", \"fill_radius\": " << opt.ortho_fill
        << ", \"contributors\": " << m.contributors << ", \"occupied\": " << m.occupied << ", \"filled\": " << m.filled << "}\n";
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the orthographic map's frame.");
    std::cout << "Orthographic map saved to: " << stem << "ortho_*.npy and ortho_frame.json, " << m.frame.width << " x " << m.frame.height
              << " pixels, " << m.occupied << " occupied, " << m.filled << " filled" << std::endl;
    if (!opt.compare_map.empty()) {  // the comparison drawn on the map: distance[index], status[index]
      std::vector<float> change(m.index.size(), 0.0f);
      std::vector<uint8_t> change_status(m.index.size(), 0);
      for (size_t p = 0; p < m.index.size(); ++p) {
        if (m.index[p] == 0xFFFFFFFFu) continue;
        if (m.index[p] >= compare_.status.size())
          throw std::runtime_error("the orthographic map's index layer names row " + std::to_string(m.index[p]) + " of a map of " +
                                   std::to_string(compare_.status.size()) + " points: the change layers cannot be drawn");
        change[p] = compare_.distance[m.index[p]];
        change_status[p] = compare_.status[m.index[p]];
      }
      writeNpy(stem + "change.npy", "<f4", {h, w}, change.data(), change.size() * 4);
      writeNpy(stem + "change_status.npy", "|u1", {h, w}, change_status.data(), change_status.size());
      std::cout << "Orthographic change layers saved to: " << stem << "change.npy, change_status.npy" << std::endl;
    }
    if (opt.crack_fuse) ortho_index = std::move(m.index);
  }

  // --orthoDefects 1: the surface defects of the finished map on `dev` (DESIGN.md "Surface defects on ortho maps"), as
  // <stem>ortho_defect_dev.npy (quanta of 2^-20 m), ortho_defect_class.npy, ortho_defect_region.npy and defects.json: the
  // parameters, the counts and one object per kept region with the metres derived from the library's integers
  void writeOrthoDefects(Device &dev, const pcp_ortho_frame &frame, const std::string &stem) {
    OrthoDefects d;
    {
      Phase ph("ortho_defects_gpu_s");
      d = dev.orthoDefects(opt.defect);
      dev.orthoDefectsFetch(d);
    }
    Phase ph_w("ortho_defects_write_s");
    fs::create_directories(fs::path(stem));
    const size_t h = static_cast<size_t>(frame.height), w = static_cast<size_t>(frame.width);
    writeNpy(stem + "ortho_defect_dev.npy", "<i4", {h, w}, d.dev.data(), d.dev.size() * 4);
    writeNpy(stem + "ortho_defect_class.npy", "|u1", {h, w}, d.cls.data(), d.cls.size());
    writeNpy(stem + "ortho_defect_region.npy", "<i4", {h, w}, d.region.data(), d.region.size() * 4);
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.9g", v);
      return std::string(b);
    };
    const double g = static_cast<double>(frame.gsd), q = 1.0 / 1048576.0;
    std::ofstream f(stem + "defects.json");
    f << "{\"threshold\": " << num(opt.defect.threshold) << ", \"window\": " << opt.defect.window_px << ", \"refine\": " << opt.defect.refine
      << ", \"min_support\": " << opt.defect.min_support << ", \"min_pixels\": " << opt.defect.min_pixels << ", \"classes\": " << opt.defect.classes
      << ", \"gsd\": " << num(g) << ", \"width\": " << frame.width << ", \"height\": " << frame.height << ", \"counts\": [";
    for (int k = 0; k < 8; ++k) f << (k ? ", " : "") << d.counts[k];
    f << "], \"regions\": [";
    const size_t rows = d.rows.size() / 16;
    for (size_t r = 0; r < rows; ++r) {
      const int64_t *t = d.rows.data() + 16 * r;
      const double px = static_cast<double>(t[1]);
      f << (r ? ",\n " : "\n ") << "{\"id\": " << r + 1 << ", \"kind\": \"" << (t[0] == 1 ? "hollow" : "bulge") << "\", \"pixels\": " << t[1]
        << ", \"area_m2\": " << num(px * g * g) << ", \"volume_m3\": " << num(static_cast<double>(t[3]) * q * g * g) << ", \"depth_m\": "
        << num(static_cast<double>(t[4]) * q) << ", \"depth_px\": [" << t[5] % frame.width << ", " << t[5] / frame.width << "], \"box_px\": ["
        << t[6] << ", " << t[8] << ", " << t[7] << ", " << t[9] << "], \"centroid_px\": [" << num(static_cast<double>(t[10]) / px) << ", "
        << num(static_cast<double>(t[11]) / px) << "], \"measured_fraction\": " << num(static_cast<double>(t[2]) / px) << ", \"open_pixels\": "
        << t[12] << ", \"first_pass_pixels\": " << t[14] << ", \"row\": [";
      for (int k = 0; k < 16; ++k) f << (k ? ", " : "") << t[k];
      f << "]}";
    }
    f << (rows ? "\n]}\n" : "]}\n");
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the surface defects of the orthographic map.");
    std::cout << "Surface defects saved to: " << stem << "ortho_defect_*.npy and defects.json, " << d.counts[0] << " regions kept, " << d.counts[1]
              << " dropped, " << d.counts[2] << " hollow and " << d.counts[3] << " bulge pixels" << std::endl;
  }

  // --orthoTexture k: the orthophoto of the finished map on `dev`, as <out>ortho/ortho_photo_*.npy and ortho_photo.json.  One call
  // of at most 2^28 fine pixels covers a band of whole map rows; the bands' rows are appended to the files in order.
  // cyl: the map is a cylinder's unrolled one (--orthoTextureCylinders 1): the same files by pcp_ortho_texture_cyl.
  void writeOrthoPhoto(Device &dev, const pcp_ortho_frame &frame, const std::string &stem, bool cyl = false) {
    Phase ph("ortho_texture_s");
    fs::create_directories(fs::path(stem));
    const int64_t k = opt.ortho_texture, W = frame.width, H = frame.height;
    const size_t fh = static_cast<size_t>(H * k), fw = static_cast<size_t>(W * k);
    const int64_t band = std::min<int64_t>(H, (int64_t(1) << 28) / (W * k * k));  // (W <= 16384, k <= 16: at least 64 rows)
    std::ofstream rgb(stem + "ortho_photo_rgb.npy", std::ios::binary), mask(stem + "ortho_photo_mask.npy", std::ios::binary),
        view(stem + "ortho_photo_view.npy", std::ios::binary), status(stem + "ortho_photo_status.npy", std::ios::binary);
    writeNpyHead(rgb, "|u1", {fh, fw, 3});
    writeNpyHead(mask, "|u1", {fh, fw});
    writeNpyHead(view, "<i2", {fh, fw});
    writeNpyHead(status, "|u1", {fh, fw});
    int64_t surface = 0, textured = 0, unseen = 0, skipped = 0, calls = 0;
    for (int64_t y0 = 0; y0 < H; y0 += band, ++calls) {
      pcp_ortho_texture_params p{};
      p.scale = static_cast<int32_t>(k);
      p.x0 = 0;
      p.y0 = static_cast<int32_t>(y0);
      p.w = static_cast<int32_t>(W);
      p.h = static_cast<int32_t>(std::min(band, H - y0));
      p.views = opt.ortho_texture_views;
      p.interpolate = opt.ortho_texture_interp ? 1 : 0;
      p.max_step = opt.ortho_texture_step;
      const OrthoPhoto part = cyl ? dev.orthoTextureCyl(p) : dev.orthoTexture(p);
      rgb.write(reinterpret_cast<const char *>(part.rgb.data()), static_cast<std::streamsize>(part.rgb.size()));
      mask.write(reinterpret_cast<const char *>(part.mask.data()), static_cast<std::streamsize>(part.mask.size()));
      view.write(reinterpret_cast<const char *>(part.view.data()), static_cast<std::streamsize>(part.view.size() * 2));
      status.write(reinterpret_cast<const char *>(part.status.data()), static_cast<std::streamsize>(part.status.size()));
      surface += part.surface;
      textured += part.textured;
      unseen += part.unseen;
      skipped += part.skipped_pairs;
    }
    rgb.close();
    mask.close();
    view.close();
    status.close();
    if (!rgb || !mask || !view || !status) throw std::runtime_error("Couldn't save the orthophoto to: " + stem);
    std::ofstream f(stem + "ortho_photo.json");
    char gsd[64], step[64];
    std::snprintf(gsd, sizeof(gsd), "%.9g", static_cast<double>(frame.gsd / static_cast<float>(k)));
    std::snprintf(step, sizeof(step), "%.9g", static_cast<double>(opt.ortho_texture_step));
    f << "{\"scale\": " << k << ", \"views\": " << opt.ortho_texture_views << ", \"interpolate\": " << (opt.ortho_texture_interp ? 1 : 0)
      << ", \"max_step\": " << step << ", \"gsd\": " << gsd << ", \"width\": " << fw << ", \"height\": " << fh << ", \"calls\": " << calls
      << ", \"surface\": " << surface << ", \"textured\": " << textured << ", \"unseen\": " << unseen << ", \"skipped_pairs\": " << skipped
      << "}\n";
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the orthophoto's description.");
    std::cout << "Orthophoto saved to: " << stem << "ortho_photo_*.npy and ortho_photo.json, " << fw << " x " << fh << " pixels, " << textured
              << " textured, " << unseen << " unseen" << std::endl;
  }

  // --crackSkeleton 1: every crack's level-set diagram on the map: nodes, edges, ends, junctions, loops and skeleton length
  void writeCrackSkeleton(const CrackSkeleton &c, const CrackMap &m, const std::string &stem) {
    Phase ph("crack_skeleton_write_s");
    const size_t nodes = c.ids.size(), edges = c.edges.size() / 3, cracks = c.cracks.size() / 6;
    writeNpy(stem + "map_crack_node.npy", "<i4", {c.node.size()}, c.node.data(), c.node.size() * 4);
    writeNpy(stem + "crack_nodes.npy", "<i8", {nodes, 10}, c.nodes.data(), c.nodes.size() * 8);
    writeNpy(stem + "crack_node_ids.npy", "<i4", {nodes}, c.ids.data(), nodes * 4);
    writeNpy(stem + "crack_edges.npy", "<i8", {edges, 3}, c.edges.data(), c.edges.size() * 8);
    if (cracks != m.ids.size()) throw std::runtime_error("The skeletons' cracks are not those of the map.");
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.9g", v);
      return std::string(b);
    };
    const std::vector<double> length = c.skeletonLengths();
    std::vector<std::string> end_xyz(cracks), junction_xyz(cracks);  // the centroids, by ascending node row
    for (size_t r = 0; r < nodes; ++r) {
      const int64_t *row = c.nodes.data() + 10 * r;
      if (row[9] != 1 && row[9] < 3) continue;
      std::string &list = row[9] == 1 ? end_xyz[static_cast<size_t>(row[0])] : junction_xyz[static_cast<size_t>(row[0])];
      list += (list.empty() ? "[" : ", [") + num(c.centroid(r, 0)) + ", " + num(c.centroid(r, 1)) + ", " + num(c.centroid(r, 2)) + "]";
    }
    std::ofstream f(stem + "crack_skeleton_3d.json");
    f << "[";
    for (size_t r = 0; r < cracks; ++r) {
      const int64_t *row = c.cracks.data() + 6 * r;
      f << (r ? ",\n " : "\n ") << "{\"id\": " << m.ids[r] << ", \"nodes\": " << row[0] << ", \"edges\": " << row[1] << ", \"ends\": " << row[2]
        << ", \"junctions\": " << row[3] << ", \"loops\": " << row[4] << ", \"skeleton_length_m\": " << num(length[r]) << ", \"end_xyz\": ["
        << end_xyz[r] << "], \"junction_xyz\": [" << junction_xyz[r] << "]}";
    }
    f << "\n]\n";
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the crack skeletons of the map.");
    std::cout << "Crack skeletons on the map saved to: " << stem << "map_crack_node.npy, crack_nodes.npy, crack_node_ids.npy, crack_edges.npy and "
              << "crack_skeleton_3d.json, " << cracks << " cracks, " << nodes << " nodes, " << edges << " edges" << std::endl;
  }

  // The direction fields of a record of crack_directions_3d.json and of a branch of crack_branches_3d.json, from the five
  // doubles of pcp_crack_axis_host (ax: links, the unit axis, its anisotropy) and the facet of the crack (with --facets 1):
  // "axis": .., "anisotropy": .., "inclination_deg": .., "class": ".." and then "facet", "facet_kind", "out_of_plane_deg",
  // "to_axis_deg", "cylinder_class" where they apply
  std::string directionFields(const double *ax, int32_t facet_id) const {
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.9g", v);
      return std::string(b);
    };
    const double deg = 180.0 / 3.14159265358979323846;
    auto cosine = [](const double *a, double bx, double by, double bz) {  // |a . b| of two unit vectors, at most 1
      return std::min(1.0, std::fabs((a[0] * bx + a[1] * by) + a[2] * bz));
    };
    std::ostringstream f;
    const bool has = ax[1] != 0.0 || ax[2] != 0.0 || ax[3] != 0.0;
    const double incl = has ? std::acos(cosine(ax + 1, opt.crack_up[0], opt.crack_up[1], opt.crack_up[2])) * deg : 0.0;
    f << "\"axis\": [" << num(ax[1]) << ", " << num(ax[2]) << ", " << num(ax[3]) << "], \"anisotropy\": " << num(ax[4]) << ", \"inclination_deg\": "
      << num(incl) << ", \"class\": \"" << (!has ? "none" : incl < 22.5 ? "vertical" : incl > 67.5 ? "horizontal" : "diagonal") << "\"";
    if (opt.facets) {
      const int32_t id = facet_id;
      const size_t fr = id < 0 ? facets_.ids.size() : static_cast<size_t>(std::lower_bound(facets_.ids.begin(), facets_.ids.end(), id) - facets_.ids.begin());
      const bool known = fr < facets_.ids.size() && facets_.ids[fr] == id;
      const bool plane = known && facets_.planar[fr];
      const bool cylinder = known && !plane && opt.facet_cylinders && fr < facet_kind_.size() && facet_kind_[fr] == 2;
      f << ", \"facet\": " << id << ", \"facet_kind\": \"" << (plane ? "plane" : cylinder ? "cylinder" : "none") << "\"";
      if (plane && has) {
        const double *pl = facets_.plane.data() + 7 * fr;
        f << ", \"out_of_plane_deg\": " << num(std::asin(cosine(ax + 1, pl[3], pl[4], pl[5])) * deg);
      }
      if (cylinder && has) {
        const pcp_cyl_frame &cy = facet_cyl_[fr];
        const double to_axis = std::acos(cosine(ax + 1, cy.a[0], cy.a[1], cy.a[2])) * deg;
        f << ", \"to_axis_deg\": " << num(to_axis) << ", \"cylinder_class\": \""
          << (to_axis < 22.5 ? "longitudinal" : to_axis > 67.5 ? "circumferential" : "diagonal") << "\"";
      }
    }
    return f.str();
  }

  // --crackBranches 1: every crack arm by arm: the branch of every point, the tables, and one record per crack with its branches
  void writeCrackBranches(const CrackBranches &c, const CrackMap &m, const std::vector<int32_t> &crack_facet, const std::string &stem) {
    Phase ph("crack_branches_write_s");
    const size_t rows = c.ids.size(), cracks = c.cracks.size() / 7;
    writeNpy(stem + "map_crack_branch.npy", "<i4", {c.branch.size()}, c.branch.data(), c.branch.size() * 4);
    writeNpy(stem + "crack_branches.npy", "<i8", {rows, 15}, c.rows.data(), c.rows.size() * 8);
    writeNpy(stem + "crack_branch_ids.npy", "<i4", {rows}, c.ids.data(), rows * 4);
    writeNpy(stem + "crack_branch_moments.npy", "<i8", {rows, 20}, c.moments.data(), c.moments.size() * 8);
    if (cracks != m.ids.size()) throw std::runtime_error("The branches' cracks are not those of the map.");
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.9g", v);
      return std::string(b);
    };
    const double unit = 1.0 / 1048576.0;  // quanta of 2^-20 m to metres
    std::vector<std::string> list(cracks);  // the branches of every crack, by ascending branch row
    for (size_t b = 0; b < rows; ++b) {
      const int64_t *row = c.rows.data() + 15 * b;
      const size_t r = static_cast<size_t>(row[0]);
      std::string &s = list[r];
      s += (s.empty() ? "\n  {" : ",\n  {");
      s += "\"id\": " + std::to_string(c.ids[b]) + ", \"points\": " + std::to_string(row[6]) + ", \"length_m\": " + num(c.length_m[b]) +
           ", \"mean_width\": " + num(c.meanWidth(b)) + ", \"min_width\": " + num(static_cast<double>(row[8]) * unit) + ", \"max_width\": " +
           num(static_cast<double>(row[9]) * unit) + ", \"arc_from_m\": " + num(static_cast<double>(row[10]) * unit) + ", \"arc_to_m\": " +
           num(static_cast<double>(row[11]) * unit) + ", \"attachments\": " + std::to_string(row[3]) + ", \"centroid\": [" + num(c.centroid(b, 0)) +
           ", " + num(c.centroid(b, 1)) + ", " + num(c.centroid(b, 2)) + "], " + directionFields(c.axis.data() + 5 * b, crack_facet[r]) + "}";
    }
    std::ofstream f(stem + "crack_branches_3d.json");
    f << "[";
    for (size_t r = 0; r < cracks; ++r) {
      const int64_t *row = c.cracks.data() + 7 * r;
      f << (r ? ",\n " : "\n ") << "{\"id\": " << m.ids[r] << ", \"branch_count\": " << row[0] << ", \"bridges\": " << row[1] << ", \"junctions_kept\": "
        << row[2] << ", \"ends_kept\": " << row[3] << ", \"pruned_branches\": " << row[4] << ", \"pruned_nodes\": " << row[5]
        << ", \"pruned_points\": " << row[6] << ", \"kept_length_m\": " << num(c.kept_length_m[r]) << ", \"branches\": [" << list[r] << "]}";
    }
    f << "\n]\n";
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the crack branches of the map.");
    std::cout << "Crack branches on the map saved to: " << stem << "map_crack_branch.npy, crack_branches.npy, crack_branch_ids.npy, "
              << "crack_branch_moments.npy and crack_branches_3d.json, " << cracks << " cracks, " << rows << " branches, " << c.pruned_branches
              << " pruned (step " << num(c.step) << " m, prune " << num(c.prune) << " m)" << std::endl;
  }

  // --crackDirection 1: every crack point's tangent, and every crack's axis against the vertical and against its facet
  void writeCrackDirections(const CrackDirections &c, const std::vector<int32_t> &crack_facet, const std::string &stem) {
    Phase ph("crack_direction_write_s");
    const size_t n = c.anisotropy.size();
    writeNpy(stem + "map_tangent.npy", "<f4", {n, 3}, c.tangent.data(), 3 * n * 4);
    writeNpy(stem + "map_anisotropy.npy", "<f4", {n}, c.anisotropy.data(), n * 4);
    std::ofstream f(stem + "crack_directions_3d.json");
    f << "[";
    for (size_t r = 0; r < c.ids.size(); ++r) {
      const double *ax = c.axis.data() + 5 * r;
      f << (r ? ",\n " : "\n ") << "{\"id\": " << c.ids[r] << ", \"links\": " << static_cast<long long>(ax[0]) << ", "
        << directionFields(ax, opt.facets ? crack_facet[r] : -1) << "}";
    }
    f << "\n]\n";
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the crack directions of the map.");
    std::cout << "Crack directions on the map saved to: " << stem << "map_tangent.npy, map_anisotropy.npy and crack_directions_3d.json, "
              << c.ids.size() << " cracks" << std::endl;
  }

  // --crackLength 1: every crack's geodesic length, ends and centreline on the map, and every point's arc position
  void writeCrackLengths(const CrackLengths &c, const std::string &stem) {
    Phase ph("crack_length_write_s");
    writeNpy(stem + "map_crack_pos.npy", "<u8", {c.pos.size()}, c.pos.data(), c.pos.size() * 8);
    writeNpy(stem + "crack_paths.npy", "<i4", {c.path.size()}, c.path.data(), c.path.size() * 4);
    writeNpy(stem + "crack_path_offsets.npy", "<i8", {c.offsets.size()}, c.offsets.data(), c.offsets.size() * 8);
    std::ofstream f(stem + "crack_lengths_3d.json");
    auto num = [](double v) {
      char b[64];
      std::snprintf(b, sizeof(b), "%.9g", v);
      return std::string(b);
    };
    const double unit = 1.0 / 1048576.0, mm = 1000.0 / 1048576.0;  // 2^-20 m to metres and to millimetres
    auto point = [&](int64_t i) {
      const size_t k = static_cast<size_t>(i);
      return "[" + num(cloud.x[k]) + ", " + num(cloud.y[k]) + ", " + num(cloud.z[k]) + "]";
    };
    f << "[";
    for (size_t r = 0; r < c.ids.size(); ++r) {
      const int64_t *row = c.rows.data() + 7 * r;
      f << (r ? ",\n " : "\n ") << "{\"id\": " << c.ids[r] << ", \"length_m\": " << num(static_cast<double>(row[2]) * unit) << ", \"hops\": " << row[3]
        << ", \"end_a\": " << row[0] << ", \"end_b\": " << row[1] << ", \"end_a_xyz\": " << point(row[0]) << ", \"end_b_xyz\": " << point(row[1])
        << ", \"path_width_mean_mm\": " << num(static_cast<double>(row[4]) / static_cast<double>(row[3] + 1) * mm)
        << ", \"path_width_min_mm\": " << num(static_cast<double>(row[5]) * mm) << ", \"path_width_max_mm\": " << num(static_cast<double>(row[6]) * mm)
        << "}";
    }
    f << "\n]\n";
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the crack lengths of the map.");
    std::cout << "Crack lengths on the map saved to: " << stem << "map_crack_pos.npy, crack_paths.npy, crack_path_offsets.npy and crack_lengths_3d.json, "
              << c.ids.size() << " cracks, " << c.path.size() << " path points" << std::endl;
  }

  // --balanceExposure 1: the staged colour stage with the exposure gains between the colour pass and the finalise, and the
  // gains on record next to the outputs
  // (fetch = false, --skip_full_cloud 1: the result stays on the device)
  void colorizeBalanced(std::vector<uint8_t> &rgb, std::vector<uint8_t> &has, bool fetch = true) {
    Colorizer col(gpu->device(0));
    col.accumulate();
    const std::vector<double> gains = col.balanceExposure();
    if (fetch)
      col.finalise(rgb, has);
    else
      col.finaliseOnDevice();
    const std::string path = opt.outputPath + "exposure_gains.txt";
    std::ofstream f(path);
    for (size_t k = 0; k < keyframes.size(); ++k) {
      char g[64];
      std::snprintf(g, sizeof(g), "%.9g", gains[k]);
      f << std::to_string(keyframes[k].imageTimestamp) << " " << g << "\n";
    }
    f.close();
    if (!f) throw std::runtime_error("Couldn't save the exposure gains.");
    std::cout << "Exposure gains saved to: " << path << std::endl;
  }

  void pcdColorizationAndSmooth() {  // :474-602
    uploadImages(true);
    if (opt.crack_maps) writeCrackMaps();
    if (opt.crack_width) writeCrackWidth();
    std::vector<float> wx, wy, wz;  // cloudInWorldWithRGBandMask
    std::vector<float> wxyz;
    std::vector<uint8_t> wrgb;
    std::vector<uint16_t> wmask;
    if (opt.fuse_masks) {
      // every keyframe's mask takes part in the fusion: a missing one ends the run (the reference ends with -2 too, :776-781
      // and the writer's exception)
      for (size_t k = 0; k < keyframes.size(); ++k)
        if (mask_missing[k]) throw std::runtime_error("Failed to read image from: " + keyframes[k].maskImagePath);
      gpu->setLabelFusion(true);
    }
    if (enableMaskSegmentation && !(opt.fuse_masks && opt.skip_filtered_dumps)) {
      for (size_t k = 0; k < keyframes.size(); ++k) {
        VisiblePoints v;
        if (mask_missing[k])  // :779-780: message, empty scanInBodyWithRGBandMask -> PCDWriter throws below (exit -2)
          std::cout << "Failed to read image from: " << keyframes[k].maskImagePath << std::endl;
        else {
          Phase ph("frame_visible_gpu_s");
          v = gpu->frameVisible(static_cast<int>(k));
        }
        Phase ph_w("rgb_mask_dumps_write_ascii_s");
        const std::string path =
            opt.outputPath + "filtered_pcd/" + std::to_string(keyframes[k].imageTimestamp) + "_rgb-mask" + ".pcd";
        if ((opt.device_writer ? deviceWriteRows(gpu->device(0), path, ChunkedAsciiWriter::XYZRGBMask, PCP_ROWS_XYZRGBMASK, v.index.size(),
                                                 v.xyz_cam.data(), v.rgb.data(), v.mask.data())
                               : writeASCII_XYZRGBMask(path, v.xyz_cam.data(), v.rgb.data(), v.mask.data(), v.index.size())) == -1)
          throw std::runtime_error("Couldn't save filtered point cloud to PCD file.");
        std::cout << "Filtered point cloud saved to: " << path << ", the point size is " << v.index.size() << std::endl;
        if (opt.fuse_masks || opt.skip_full_cloud) continue;  // the fused file has one row per map point, and
                                                              // --skip_full_cloud 1 writes neither: no concatenation
        wxyz.insert(wxyz.end(), v.xyz_world.begin(), v.xyz_world.end());
        wrgb.insert(wrgb.end(), v.rgb.begin(), v.rgb.end());
        wmask.insert(wmask.end(), v.mask.begin(), v.mask.end());
      }
    }
    std::vector<uint8_t> rgb, has;
    if (opt.skip_full_cloud) {
      // --skip_full_cloud 1 (one GPU, --outputLeaf given): the same colour result, left on the device; only the voxel rows leave it
      Device &dev = gpu->device(0);
      {
        Phase ph("colourise_gpu_s");
        if (opt.balance_exposure)
          colorizeBalanced(rgb, has, false);
        else
          dev.check(pcp_colorize(dev.get(), nullptr, nullptr));
      }
      if (opt.smooth_colors_radius > 0.0f) {
        Phase ph("colour_smooth_gpu_s");
        int64_t coloured = 0;
        dev.check(pcp_colour_smooth_local(dev.get(), opt.smooth_colors_radius, &coloured));
      }
      reduceToVoxels();
      if (!opt.compare_map.empty()) writeCompare();
      if (opt.facets) writeFacets();
      if (opt.ortho_map) opt.ortho_by_facet ? writeOrthoMapsByFacet() : writeOrthoMap();
      if (opt.crack_fuse) writeCrackFuse();
      return;
    }
    {
      Phase ph("colourise_gpu_s");
      if (opt.balance_exposure)
        colorizeBalanced(rgb, has);
      else
        gpu->colorize(rgb, has);  // smoothColors + removePointsWithNoColor flag
    }
    if (opt.smooth_colors_radius > 0.0f) {  // smoothColorsWithLocalRegion(rgbCloud, r), :597
      Phase ph("colour_smooth_gpu_s");
      gpu->smoothColorsWithLocalRegion(opt.smooth_colors_radius, rgb, has);
    }
    if (opt.output_leaf > 0.0f) reduceToVoxels();  // (of the colour result as it lies on the device now)
    if (!opt.compare_map.empty()) writeCompare();   // (it reads the raw map; before --facets, whose partition ends with a new estimate of the normals)
    if (opt.facets) writeFacets();                  // (it reads the raw map; the colour result stays as it is)
    if (opt.ortho_map) opt.ortho_by_facet ? writeOrthoMapsByFacet() : writeOrthoMap();  // (likewise; before --crackFuse, whose layers it gathers by the index layer)
    if (opt.crack_fuse) writeCrackFuse();           // (it reads the raw map and the masks; the colour result stays as it is)
    std::vector<uint8_t> label;
    if (opt.fuse_masks) {
      Phase ph("labels_gpu_s");
      gpu->labels(label);  // of the colour result above; the local smoothing leaves them alone
    }
    Phase ph_w("final_pcd_write_ascii_s");
    if (opt.device_writer) {
      // the same two files from the colour result where it lies (after --smoothColorsRadius: the smoothed one): no row is
      // gathered or formatted on the host; the concatenated mask samples of a run without --fuseMasks are host arrays
      int64_t coloured = 0;
      for (size_t i = 0; i < cloud.size(); ++i) coloured += has[i] ? 1 : 0;
      const bool mask_rows = opt.fuse_masks ? coloured > 0 : !wmask.empty();
      if (enableMaskSegmentation && mask_rows) {
        Phase ph_m("mask_pcd_rows_s");
        const std::string path = opt.outputPath + "cloudInWorldWithRGBandMask.pcd";
        if ((opt.fuse_masks ? deviceWriteColoured(path, true, coloured)
                            : deviceWriteRows(gpu->device(0), path, ChunkedAsciiWriter::XYZRGBMask, PCP_ROWS_XYZRGBMASK, wmask.size(),
                                              wxyz.data(), wrgb.data(), wmask.data())) == -1)
          throw std::runtime_error("Couldn't save colorized and segment colored point cloud.");
        std::cout << "All colored and segment colored cloud saved to: " << path << std::endl;
      }
      if (coloured > 0) {
        const std::string path = opt.outputPath + "cloudInWorldWithRGB.pcd";
        if (deviceWriteColoured(path, false, coloured) == -1) throw std::runtime_error("Couldn't save colorized point cloud.");
        std::cout << "All colored cloud saved to: " << path << std::endl;
      }
      return;
    }
    XYZICloud out;
    std::vector<uint8_t> out_rgb;
    for (size_t i = 0; i < cloud.size(); ++i)
      if (has[i]) {
        out.push_back(cloud.x[i], cloud.y[i], cloud.z[i], 0.0f);
        out_rgb.insert(out_rgb.end(), {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]});
        if (opt.fuse_masks) {  // the same rows, the map point itself, its fused label
          wxyz.insert(wxyz.end(), {cloud.x[i], cloud.y[i], cloud.z[i]});
          wmask.push_back(label[i]);
        }
      }
    if (opt.fuse_masks) wrgb = out_rgb;
    if (enableMaskSegmentation && !wmask.empty()) {  // saveColorizedPointCloud(rgbCloud, withMask), :933-960
      Phase ph_m("mask_pcd_rows_s");  // (inside final_pcd_write_ascii_s)
      const std::string path = opt.outputPath + "cloudInWorldWithRGBandMask.pcd";
      if (writeASCII_XYZRGBMask(path, wxyz.data(), wrgb.data(), wmask.data(), wmask.size()) == -1)
        throw std::runtime_error("Couldn't save colorized and segment colored point cloud.");
      std::cout << "All colored and segment colored cloud saved to: " << path << std::endl;
    }
    if (out.size() > 0) {  // :912-929
      const std::string path = opt.outputPath + "cloudInWorldWithRGB.pcd";
      if (writeASCII_XYZRGB(path, out.x.data(), out.y.data(), out.z.data(), out_rgb.data(), out.size()) == -1)
        throw std::runtime_error("Couldn't save colorized point cloud.");
      std::cout << "All colored cloud saved to: " << path << std::endl;
    }
  }
};

int main(int argc, char **argv) {
  const auto t_main = PhaseClock::clock::now();
  // Decoded keyframes are 6-37 MB buffers that live for one upload each.  glibc serves such sizes by mmap / munmap until a
  // freed block has raised its threshold: sixteen decoder threads then fault fresh pages in and tear mappings down while this
  // thread's uploads pin and unpin theirs -- all under one address-space lock.  Measured (profiles/r05_cli_e2e_probe_before.log / _after.log, profiles/cli_e2e_probe.py): the
  // 32 uploads of a 1 M-point / 32-keyframe run took 0.50 s when nothing large had been freed before (--skip_filtered_dumps 1)
  // and 0.03 s otherwise.  The threshold is set up front: the buffers come from the heaps and are reused.
  (void)mallopt(M_MMAP_THRESHOLD, 32 << 20);   // (glibc's ceiling)
  (void)mallopt(M_TRIM_THRESHOLD, 1 << 30);
  struct TimingAtExit {  // also after an exception: the phases reached so far
    PhaseClock::clock::time_point t0;
    ~TimingAtExit() {
      if (const char *path = std::getenv("PCP_CLI_TIMING")) g_clock.write(path, PhaseClock::since(t0));
    }
  } timing_at_exit{t_main};
  try {
    const Options o = parse(argc, argv);
    if (o.help) {
      usage(std::cout);
      return 1;
    }
    if (o.have_p && o.have_o && o.have_i) {
      Processor processor(o);
      processor.process();
      std::cout << "Processing completed successfully." << std::endl;
    } else {
      std::cerr << "Error: Missing required arguments." << std::endl;
      usage(std::cerr);
      return -1;
    }
  } catch (const std::exception &e) {
    std::cerr << "Unhandled Exception reached the top of main: " << e.what() << ", application will now exit"
              << std::endl;
    return -2;
  }
  return 0;
}
