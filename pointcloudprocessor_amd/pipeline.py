"""Host-side mirror of the reference's operator interface for the hot path, on
top of the C ABI (capi.py).  Names follow the reference:

  ViewCulling.cull            vlcal::ViewCulling::cull     (view_culling.hpp:34)
  PointCloudColorizer.run     pcdColorizationAndSmooth     (PointCloudProcessor.cpp:474-602)
  CloudSmooth.process         CloudSmooth::process         (cloudSmooth.cpp:77-185)

plus the point-index sharding of SURVEY.md section 8(e): every rank owns a
contiguous slice of the map, all keyframes / images are replicated, and the one
exchange step is an all-reduce(MIN) of the per-keyframe depth maps.  Per-point
results (top-5 lists, colours) are rank-local, so no other collective is on the
data path; outputs are assembled with an all-gather when asked for.

The compute engine is libpcp_hip.so; there is no CPU engine in this package.
"""
from __future__ import annotations

import numpy as np

from . import capi


MAX_UPLOAD_POINTS = (1 << 31) - 1  # pcp_upload_cloud*: n < 2^31


def shard_bounds(n: int, rank: int, world: int):
    """Contiguous index range of `rank` (first n % world ranks get one extra point)."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class _DeviceArray:
    """Minimal __cuda_array_interface__ carrier for a raw device pointer."""

    def __init__(self, ptr: int, n: int, typestr: str = "<f4"):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class HipEngine:
    """One GPU worth of the hot path (one pcp_context)."""

    def __init__(self, device: int = 0):
        self.ctx = capi.Context(device)
        self.device = device

    def configure(self, camera: dict | capi.Camera, cull: capi.CullParams | None = None):
        cam = camera if isinstance(camera, capi.Camera) else capi.camera_from_dict(camera)
        self.ctx.set_camera(cam, cull)
        self.match_mode = capi.MATCH_ROUNDTRIP if cull is None else int(cull.match_mode)

    def upload_cloud(self, x, y, z):
        self.ctx.upload_cloud(x, y, z)

    def set_keyframes(self, poses, images=None, masks=None, T_opt=None, balance="keep"):
        """balance: the keyframe colour balance of the images uploaded from now on (capi.Context.set_image_balance: True for
        the defaults, a dict of capi.balance_params()'s arguments, None for off); "keep" leaves the context's setting."""
        self.ctx.set_frames(poses, T_opt)
        import numpy as np

        pos = np.asarray(poses, np.float64).reshape(-1, 7)[:, :3]
        self.mean_keyframe_position = pos.mean(axis=0) if len(pos) else None  # (the viewer of ortho_maps_by_facet's frames)
        self.keyframe_positions = pos  # (compare_map's default viewer is their mean)
        if not (isinstance(balance, str) and balance == "keep"):
            self.ctx.set_image_balance(balance)
        if images is not None:
            for f, im in enumerate(images):
                self.ctx.upload_image(f, im)
        if masks is not None:
            for f, m in enumerate(masks):
                if m is not None:
                    self.ctx.upload_mask(f, m)

    def use_torch_stream(self):
        """Run the library's kernels on torch's current HIP stream: the collective is then
        stream-ordered against them (RCCL waits on / is waited for through events), with no
        host synchronisation between the depth pass, the all-reduce and the colour pass."""
        import torch

        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        self._on_torch_stream = True

    # hooks used by the sharded driver
    @property
    def n_frames(self):
        return self.ctx.n_frames

    def depth_pass(self, f0: int = 0, f1: int | None = None):
        self.ctx.depth_pass(f0, f1)

    def depth_maps_tensor(self):
        """torch view (no copy) of the device-resident depth maps, for RCCL."""
        import torch

        ptr, n = self.ctx.depth_maps_device()
        if not getattr(self, "_on_torch_stream", False):
            self.ctx.synchronize()
        # the view is rebuilt whenever the library may have reallocated or re-shaped the maps (new address, length,
        # keyframe count or cull geometry); otherwise one wrapper per step would cost ~50 us of host time
        key = (ptr, n, self.ctx.n_frames, self.ctx.map_shape)
        cached = getattr(self, "_depth_tensor", None)
        if cached is None or cached[0] != key:
            self._depth_tensor = (key, torch.as_tensor(_DeviceArray(ptr, n), device=f"cuda:{self.device}"))
        return self._depth_tensor[1]

    def set_label_fusion(self, enable: bool = True):
        """Fused segmentation labels (pcp_set_label_fusion): every later colour result of this engine carries label / hits /
        views per point; every keyframe then needs its mask."""
        self.ctx.set_label_fusion(enable)
        self.fuse_labels = bool(enable)

    def labels(self):
        """dict(label, hits, views), uint8[n] each, of the latest colour result (label fusion on)."""
        return self.ctx.colour_labels()

    def colour_from_depth(self, download=True):
        return self.ctx.colorize_from_depth(download=download)

    def smooth_colours_local(self, radius: float, download: bool = True):
        """smoothColorsWithLocalRegion(rgbCloud, radius) (PointCloudProcessor.cpp:634-703, call commented out at :597) in
        place on the colour result of this context: dict(rgb (n,3) uint8, has (n,) uint8), None entries without download."""
        self.ctx.colour_smooth_local(radius)
        if not download:
            return dict(rgb=None, has=None)
        w = self.ctx.download_result_packed()
        rgb = np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], axis=1).astype(np.uint8)
        return dict(rgb=rgb, has=((w >> 24) & 1).astype(np.uint8))

    def close(self):
        self.ctx.close()


class ViewCulling:
    """vlcal::ViewCulling with the z-buffer routine (view_culling.cpp:52-174)."""

    def __init__(self, engine: HipEngine):
        self.engine = engine

    def cull(self, keyframe: int):
        """Returns (indices kept, in input order; depth map)."""
        keep, dmap, _ = self.engine.ctx.cull_frame(keyframe)
        return np.nonzero(keep)[0].astype(np.int32), dmap


class PointCloudColorizer:
    """pcdColorizationAndSmooth over a (possibly sharded) map."""

    def __init__(self, engine, rank: int = 0, world: int = 1, group=None, chunks: int = 0, balance_exposure: bool = False,
                 exposure_sigma_n: float = 10.0, exposure_sigma_g: float = 0.1):
        """balance_exposure: one brightness gain per keyframe from the map points that two keyframes both colour
        ("Exposure gains"), applied per listed view when the colours are finalised; `gains` holds them after
        run().  Off by default (the reference's behaviour).  The pair statistics are additive over index shards, but their
        exchange is not built: world > 1 raises ValueError."""
        if balance_exposure and world > 1:
            raise ValueError("balance_exposure: the pair statistics of the index shards would have to be summed across ranks, "
                             "which is not built; run it on one rank holding the whole map")
        self.engine = engine
        self.rank = rank
        self.world = world
        self.group = group
        self.chunks = chunks
        self.balance_exposure = bool(balance_exposure)
        self.exposure_sigma = (float(exposure_sigma_n), float(exposure_sigma_g))
        self.gains = None

    def _with_labels(self, out: dict, fuse_labels: bool, download: bool):
        if fuse_labels and download:
            out = dict(out, **self.engine.labels())
        return out

    def _voxel_output(self, leaf: float, fuse_labels: bool) -> dict:
        """The voxel-grid output of the colour result that was just made ("Voxel-grid output")."""
        ctx = self.engine.ctx
        ctx.voxel_reduce_begin(leaf)
        try:
            rows = ctx.voxel_reduce_add()
            ctx.voxel_reduce_finish()
            out = ctx.voxel_reduce_fetch(want_label=fuse_labels)
            out["rows"] = rows
            return out
        finally:
            ctx.voxel_reduce_end()

    def ortho_map(self, frame="auto", gsd: float = 0.01, fill_radius: int = 0, crack_map: dict | None = None, xyz=None,
                  viewer=None, texture: dict | None = None, defects: dict | None = None) -> dict:
        """One orthographic picture of the colour result run() left on the device ("Orthographic maps"): dict(index
        (H, W) uint32 with 0xFFFFFFFF for an empty pixel, depth (H, W), rgb (H, W, 3), status (H, W) 0 empty / 1 direct /
        2 filled, source (H, W), frame (the dict that takes a pixel back to world coordinates), occupied, filled,
        contributors, and label (H, W) when the run fused labels).  The nearest coloured point wins a pixel; fill_radius > 0
        fills empty pixels from their nearest occupied pixel within that many pixels.

        frame: a dict(o, u, v, n, gsd, width, height, d_min, d_max), or "auto": the plane fitted on the host
        (capi.ortho_fit_frame_host) to the coloured rows of `xyz` -- the uploaded map as the caller holds it, (n, 3) or
        (x, y, z); nothing of it is kept here -- at `gsd` metres per pixel, seen from the side of `viewer` (3 numbers, e.g.
        the mean keyframe position; None: n's largest component negative).
        crack_map: the dict crack_map() returned (None: the one its last call on this object left, when it is of this
        cloud's size): the result gains width (H, W) float32 and crack (H, W) int32, gathered on the host as width_mean[index]
        and label[index], 0 and -1 on empty pixels.
        texture: dict(scale[, views, interpolate, max_step]) -- the result gains photo, the orthophoto of the finished map at
        `scale` fine pixels per pixel and axis, coloured straight from the keyframe images ("Orthophotos"): dict(rgb
        (H scale, W scale, 3), mask, status, view, count, surface, textured, unseen, skipped_pairs).  It runs after the
        finish and the fetch, before the map ends, on the depth maps run() left.
        defects: dict(threshold[, window, refine, min_support, min_pixels, classes]) -- the result gains defect_dev (H, W) int32
        in quanta of 2^-20 m, defect_class (H, W) uint8 (1 hollow, 2 bulge), defect_region (H, W) int32 and defects, a list of
        dicts per kept region with area_m2, volume_m3, depth_m, centroid_px, measured_fraction, open_pixels and the raw row
        ("Surface defects on ortho maps").  It runs on the finished map, before the map ends.

        An index shard sees only its own points, so world > 1 raises ValueError.  (The shards' key images would merge by an
        all-reduce(MIN); not built.)"""
        if self.world > 1:
            raise ValueError("ortho_map: an index shard sees only its own points; the per-pixel keys of the shards would "
                             "have to be merged across ranks (all-reduce MIN), which is not built: run it on one rank "
                             "holding the whole map")
        texture = ortho_texture_request("ortho_map", texture)
        defects = ortho_defects_request("ortho_map", defects)
        ctx = self.engine.ctx
        if isinstance(frame, str):
            if frame != "auto":
                raise ValueError(f"ortho_map: frame {frame!r} is neither a dict nor \"auto\"")
            xyz = _rows_xyz("ortho_map", xyz, ctx.n)
            has = (ctx.download_result_packed() >> 24).astype("uint8")
            frame = capi.ortho_fit_frame_host(xyz, gsd, has=has, viewer=viewer)
        fuse_labels = bool(getattr(self.engine, "fuse_labels", False))
        ctx.ortho_begin(frame)
        try:
            contributors = ctx.ortho_add(0)
            occupied, filled = ctx.ortho_finish(fill_radius)
            out = ctx.ortho_fetch(want_label=fuse_labels)
            if texture is not None:
                out["photo"] = ctx.ortho_texture(**texture)
            if defects is not None:
                out.update(ortho_defect_layers(ctx, defects, capi.ortho_frame(frame).gsd))
        finally:
            ctx.ortho_end()
        out.update(frame=capi.ortho_frame(frame).as_dict(), contributors=contributors, occupied=occupied, filled=filled)
        if crack_map is None:
            crack_map = getattr(self, "last_crack_map", None)
            if crack_map is not None and len(crack_map["label"]) != ctx.n:
                crack_map = None  # (of a cloud that has been replaced)
        if crack_map is not None:
            out.update(ortho_crack_layers(out["index"], crack_map["width_mean"], crack_map["label"]))
        return out

    def facets(self, xyz=None, normal_radius: float = 0.1, link_radius: float = 0.1, angle_deg: float = 10.0, plane_tol: float = 0.01,
               max_curvature: float = 0.02, min_points: int = 1000, max_rms: float = 0.01, cylinders: bool = False,
               cylinder_gsd: float = 0.01, viewer=None) -> dict:
        """The planar facets of the uploaded map ("Planar facets"): the connected components of the map points
        under a link of distance, normal angle and mutual plane distance, one per face of the structure.  The normals are
        estimated at normal_radius when none of that radius are live.  dict of capi.Context.facets (label, ids, rows, box,
        facet_points, components, facets) plus, per facet, plane (F, 7) float64 -- the columns capi.FA_PLANE: centroid, unit
        normal, rms in metres, from capi.facet_plane_host -- and planar (F,) bool: rms <= max_rms and a normal that exists.
        The global test is what stops chaining: a facet that runs round a curved surface has a large rms and is flagged.

        xyz: the uploaded map as the caller holds it, (n, 3) or (x, y, z) -- a facet's integers are relative to its root point,
        whose coordinates are read from it; nothing of it is kept here.

        cylinders ("Cylindrical facets"): every facet that is not planar is fitted a cylinder from its points and
        their normals (capi.cyl_fit_host at cylinder_gsd, seen from `viewer`; None: the mean keyframe position), and the dict
        gains cylinder -- a list per facet of None (planar, or the fit was refused) or dict(frame, stats) -- and kind (F,) uint8:
        0 neither, 1 planar, 2 cylindrical (not planar, fitted, rms <= max_rms).  Without it the dict is what it always was.

        An index shard sees only its own points, so world > 1 raises ValueError.  (The forests of the shards would have to be
        united across the cells that two ranks share; not built.)"""
        import numpy as np

        if self.world > 1:
            raise ValueError("facets: an index shard sees only its own points; the union-find forests of the shards would have "
                             "to be united across ranks, which is not built: run it on one rank holding the whole map")
        ctx = self.engine.ctx
        xyz = _rows_xyz("facets", xyz, ctx.n) if xyz is not None else None
        if xyz is None:
            raise ValueError("facets: the planes are taken about each facet's root point: pass the uploaded map as xyz")
        if ctx.normals_radius != normal_radius:  # (None after an upload: the library dropped the estimate)
            ctx.estimate_normals(normal_radius)
        out = ctx.facets(link_radius, angle_deg, plane_tol, max_curvature, min_points)
        plane = np.zeros((len(out["ids"]), 7), np.float64)
        for r, (fid, row) in enumerate(zip(out["ids"], out["rows"])):
            plane[r] = capi.facet_plane_host(xyz[fid], row)
        out["plane"] = plane
        out["planar"] = (plane[:, 6] <= max_rms) & (np.abs(plane[:, 3:6]).max(axis=1, initial=0.0) > 0) if len(plane) else np.zeros(0, bool)
        if cylinders:
            if viewer is None:
                viewer = getattr(self.engine, "mean_keyframe_position", None)
            normal = ctx.normals_fetch()["normal"]
            out["cylinder"] = [None] * len(out["ids"])
            out["kind"] = out["planar"].astype(np.uint8)
            for r in np.flatnonzero(~out["planar"]):
                try:
                    frame, stats = capi.cyl_fit_host(xyz, normal, cylinder_gsd, has=(out["label"] == out["ids"][r]).astype(np.uint8),
                                                     viewer=viewer)
                except capi.PcpError as e:
                    if e.code != capi.PCP_ERR_RANGE:  # (RANGE: the facet is no cylinder this fit can give; anything else is a fault)
                        raise
                    continue
                out["cylinder"][r] = dict(frame=frame.as_dict(), stats=stats)
                if stats["rms"] <= max_rms:
                    out["kind"][r] = 2
        self.last_facets = out
        return out

    def ortho_maps_by_facet(self, gsd: float, xyz=None, facets: dict | None = None, fill_radius: int = 0, viewer=None,
                            texture: dict | None = None, cylinders: bool = False, texture_cylinders: bool = False,
                            defects: dict | None = None) -> list:
        """One orthographic map per planar facet of the colour result run() left on the device: for every planar row of
        `facets` (the dict facets() returned; None: the one its last call on this object left) a frame fitted on the host to
        the facet's points (capi.ortho_fit_frame_host with has = (label == id)) at `gsd` metres per pixel, seen from `viewer`
        (None: the mean keyframe position), then begin / ortho_add_facet / finish / fetch / end.  Only the facet's own rows
        are drawn: a wall that crosses the frame's window does not show as a line.  A list, in the table's order, of the
        dicts ortho_map returns, each with facet (its id) and row (its row of the table).  texture: as ortho_map's.

        cylinders ("Cylindrical facets"): the cylindrical facets of a facets(..., cylinders=True) are drawn too, each
        unrolled through a cylinder fitted at `gsd` from the facet's points and the live normals (ctx.normals_fetch), and every
        map's dict carries kind (1 planar, 2 cylindrical).  texture is applied to the planar facets only, unless
        texture_cylinders is given too ("Orthophotos of unrolled maps"): then the cylindrical maps gain photo as
        well, by ctx.ortho_texture_cyl with the same request.  texture_cylinders needs both texture and cylinders.
        defects: as ortho_map's, on every map drawn, planar and cylindrical (on a cylinder the depth layer is the radial
        deviation from the fitted cylinder); every region's dict carries facet, the id of its facet.

        An index shard sees only its own points, so world > 1 raises ValueError."""
        import numpy as np

        if self.world > 1:
            raise ValueError("ortho_maps_by_facet: an index shard sees only its own points; the per-pixel keys of the shards "
                             "would have to be merged across ranks (all-reduce MIN), which is not built: run it on one rank "
                             "holding the whole map")
        texture = ortho_texture_request("ortho_maps_by_facet", texture)
        defects = ortho_defects_request("ortho_maps_by_facet", defects)
        if texture_cylinders and (texture is None or not cylinders):
            raise ValueError("ortho_maps_by_facet: texture_cylinders needs texture (the request) and cylinders=True (the maps it "
                             "textures)")
        ctx = self.engine.ctx
        facets = getattr(self, "last_facets", None) if facets is None else facets
        if facets is None or len(facets["label"]) != ctx.n:
            raise ValueError("ortho_maps_by_facet: no facets of this cloud (call facets() first)")
        xyz = _rows_xyz("ortho_maps_by_facet", xyz, ctx.n)
        if viewer is None:
            viewer = getattr(self.engine, "mean_keyframe_position", None)
        fuse_labels = bool(getattr(self.engine, "fuse_labels", False))
        maps = []
        if cylinders:
            if "kind" not in facets:
                raise ValueError("ortho_maps_by_facet: cylinders asked of facets without them (call facets(..., cylinders=True))")
            kinds = np.asarray(facets["kind"])
            normal = ctx.normals_fetch()["normal"] if (kinds == 2).any() else None
        else:
            kinds = np.asarray(facets["planar"]).astype(np.uint8)
        for row in np.flatnonzero(kinds > 0):
            fid = int(facets["ids"][row])
            member = (facets["label"] == fid).astype(np.uint8)
            if kinds[row] == 1:
                frame = capi.ortho_fit_frame_host(xyz, gsd, has=member, viewer=viewer)
                ctx.ortho_begin(frame)
                frame = capi.ortho_frame(frame).as_dict()
            else:
                frame, _ = capi.cyl_fit_host(xyz, normal, gsd, has=member, viewer=viewer)
                ctx.ortho_begin_cyl(frame)
                frame = frame.as_dict()
            try:
                contributors = ctx.ortho_add_facet(fid, 0)
                occupied, filled = ctx.ortho_finish(fill_radius)
                out = ctx.ortho_fetch(want_label=fuse_labels)
                if texture is not None and kinds[row] == 1:
                    out["photo"] = ctx.ortho_texture(**texture)
                elif texture_cylinders and kinds[row] == 2:
                    out["photo"] = ctx.ortho_texture_cyl(**texture)
                if defects is not None:
                    out.update(ortho_defect_layers(ctx, defects, frame["gsd"], facet=fid))
            finally:
                ctx.ortho_end()
            out.update(frame=frame, contributors=contributors, occupied=occupied, filled=filled, facet=fid, row=int(row))
            if cylinders:
                out["kind"] = int(kinds[row])
            maps.append(out)
        return maps

    def geometry_maps(self, frame: int, normal_radius: float = 0.1) -> dict:
        """The geometry maps of one keyframe at camera resolution, reduced on the device ("Geometry maps"):
        dict(index (H, W) int32 with -1 for an empty pixel, range (H, W), xyz_cam (H, W, 3), pixels, and -- with
        normal_radius > 0 -- normal_cam (H, W, 3)): the distance_mask / points_3d_mask / norm_mask of
        scripts/genNormAndDistanceMask.py, the nearest kept point winning a pixel.  The normals are estimated once per
        uploaded cloud and radius, over the whole map.

        An index shard sees only its own points, so world > 1 raises ValueError.  (The (range, index) keys of the shards
        would merge by an all-reduce(MIN) over the key images, the winners' rows then coming from their owners; not built.)"""
        if self.world > 1:
            raise ValueError("geometry_maps: an index shard sees only its own points; the per-pixel keys of the shards would "
                             "have to be merged across ranks (all-reduce MIN), which is not built: run it on one rank "
                             "holding the whole map")
        ctx = self.engine.ctx
        if normal_radius and ctx.normals_radius != normal_radius:  # (None after an upload: the library dropped the estimate)
            ctx.estimate_normals(normal_radius)
        return ctx.frame_geometry(frame, normals=bool(normal_radius))

    def compare_map(self, base_xyz, normal_radius: float = 0.1, radius: float = 0.03, half_length: float = 0.05, min_points: int = 5,
                    reg_error: float = 0.0, viewer=None, normals=None) -> dict:
        """The uploaded map against an earlier survey of the same structure ("Map comparison"): per map point the
        signed distance along its normal to the points of base_xyz ((n_base, 3), or (x, y, z)) inside a cylinder of `radius` and
        +-half_length, and the level of detection from the two epochs' scatter (Lague et al.'s M3C2).  Positive: the map lies
        nearer the viewer than the base (deposit, bulge), negative: loss.  The normals are `normals` ((n, 3) float32), or the
        map's own, estimated at normal_radius when none of that radius are live, and are turned towards `viewer` (None: the
        fp64 mean of the keyframes' positions, each divided by their number and summed in order, rounded to float32; without
        keyframes the normals keep their sign).  dict of capi.Context.compare: distance, lod, status, sums, direction, stats.
        The base stays on the device until capi.Context.compare_end; base_xyz None compares against the base that is there
        (register_base's, under the transform it found).  Base points the map has no counterpart for are found by a second run
        with the roles swapped.

        An index shard sees only its own points, so world > 1 raises ValueError."""
        import numpy as np

        if self.world > 1:
            raise ValueError("compare_map: an index shard sees only its own points; the candidates of a point near a shard's edge "
                             "lie with another rank, which is not built: run it on one rank holding the whole map")
        ctx = self.engine.ctx
        if isinstance(base_xyz, (tuple, list)) and len(base_xyz) == 3 and np.ndim(base_xyz[0]) == 1:
            base_xyz = np.stack([np.asarray(a, np.float32) for a in base_xyz], axis=1)
        base = None if base_xyz is None else np.asarray(base_xyz, np.float32).reshape(-1, 3)
        if viewer is None:
            poses = getattr(self.engine, "keyframe_positions", None)
            if poses is not None and len(poses):
                viewer = [0.0, 0.0, 0.0]
                for p in poses:  # (the order of operations of the host program's mean)
                    for a in range(3):
                        viewer[a] += float(p[a]) / float(len(poses))
        if normals is None and ctx.normals_radius != normal_radius:  # (None after an upload: the library dropped the estimate)
            ctx.estimate_normals(normal_radius)
        if base is not None:  # (None: the base that register_base left, under its transform)
            ctx.compare_set_base(base)
        if viewer is None:
            return ctx.compare(radius, half_length, reg_error, min_points, 0, (0.0, 0.0, 0.0), normals)
        return ctx.compare(radius, half_length, reg_error, min_points, 1, tuple(np.asarray(viewer, np.float64).astype(np.float32)), normals)

    def register_base(self, base_xyz, normal_radius: float = 0.1, normals=None, **params) -> dict:
        """Brings an earlier survey onto the uploaded map by point-to-plane ICP before it is compared ("Map
        registration"): base_xyz ((n_base, 3), or (x, y, z)) becomes the base of the comparison and is moved rigidly until its
        rows lie on the planes of their nearest map points.  The normals are `normals` ((n, 3) float32), or the map's own,
        estimated at normal_radius when none of that radius are live, exactly as compare_map does.  params: those of
        capi.register_params (match_radius, max_plane_distance, sample_stride, max_iterations, min_pairs, tolerance, cond_tol).
        dict of capi.Context.compare_register: T (4, 4) base -> map, log, status, iterations, rms, dof, pairs.  The base and its
        transform stay on the device: compare_map(None, ...) then compares against the registered base.  The rms is a
        candidate for compare_map's reg_error; nothing applies it.

        An index shard sees only its own points, so world > 1 raises ValueError."""
        import numpy as np

        if self.world > 1:
            raise ValueError("register_base: an index shard sees only its own points; the partner of a row near a shard's edge "
                             "lies with another rank, which is not built: run it on one rank holding the whole map")
        ctx = self.engine.ctx
        if isinstance(base_xyz, (tuple, list)) and len(base_xyz) == 3 and np.ndim(base_xyz[0]) == 1:
            base_xyz = np.stack([np.asarray(a, np.float32) for a in base_xyz], axis=1)
        base = np.asarray(base_xyz, np.float32).reshape(-1, 3)
        if normals is None and ctx.normals_radius != normal_radius:  # (None after an upload: the library dropped the estimate)
            ctx.estimate_normals(normal_radius)
        ctx.compare_set_base(base)
        return ctx.compare_register(normals=normals, **params)

    def _coarse_base(self, who, base_xyz, normal_radius, normals):
        import numpy as np

        if self.world > 1:
            raise ValueError(f"{who}: an index shard sees only its own points; the keypoints and partners of a base lie with every "
                             "rank, which is not built: run it on one rank holding the whole map")
        ctx = self.engine.ctx
        if isinstance(base_xyz, (tuple, list)) and len(base_xyz) == 3 and np.ndim(base_xyz[0]) == 1:
            base_xyz = np.stack([np.asarray(a, np.float32) for a in base_xyz], axis=1)
        base = np.asarray(base_xyz, np.float32).reshape(-1, 3)
        if normals is None and ctx.normals_radius != normal_radius:  # (None after an upload: the library dropped the estimate)
            ctx.estimate_normals(normal_radius)
        ctx.compare_set_base(base)
        return ctx

    def register_base_coarse(self, base_xyz, normal_radius: float = 0.1, normals=None, base_normals=None, **params) -> dict:
        """Brings an earlier survey near the uploaded map from an arbitrary pose ("Coarse registration"): base_xyz
        ((n_base, 3), or (x, y, z)) becomes the base of the comparison; spin-image descriptors at strided keypoints of both clouds
        are matched, triples of correspondences vote for a rigid motion, the winner is refitted over its inliers and set as the
        base's transform.  The map's normals are `normals` or its own, estimated at normal_radius as compare_map does; the base's
        are base_normals or estimated on the device at the same radius.  params: those of capi.coarse_params.  dict of
        capi.Context.compare_register_coarse; `runner_up` near `winner` tells a symmetric structure.  The result is good enough for
        register_base's method to finish, not for compare_map: see coarse_then_fine.

        An index shard sees only its own points, so world > 1 raises ValueError."""
        ctx = self._coarse_base("register_base_coarse", base_xyz, normal_radius, normals)
        params.setdefault("normal_radius", normal_radius)
        return ctx.compare_register_coarse(normals=normals, base_normals=base_normals, **params)

    def coarse_then_fine(self, base_xyz, normal_radius: float = 0.1, normals=None, base_normals=None, coarse=None, fine=None) -> dict:
        """register_base_coarse, then the fine registration twice from where it ended: with match_radius = 2 inlier_distance
        (the other parameters at their defaults), then with `fine` (capi.register_params; the defaults).  dict of
        capi.Context.coarse_then_fine: coarse, wide, fine, T, status.  compare_map(None, ...) then compares against the registered
        base."""
        ctx = self._coarse_base("coarse_then_fine", base_xyz, normal_radius, normals)
        coarse = dict(coarse or {})
        coarse.setdefault("normal_radius", normal_radius)
        return ctx.coarse_then_fine(normals=normals, base_normals=base_normals, coarse=coarse, fine=fine)

    def crack_width(self, frame: int, threshold: int = 0, plane_radius: int = 150,
                    want=("flags", "edges", "w2d2", "width", "points", "plane")) -> dict:
        """The crack width maps of one keyframe at camera resolution, made on the device ("Crack width maps"): per
        foreground pixel of the keyframe's mask the two edge points along the EDT direction, the plane of the position
        image's window of +-plane_radius pixels and the 3-D width between the two edge rays on that plane -- the second half
        of Crack.process() in scripts/genNormAndDistanceMask.py (compute_skeleton_edge_pts).  See capi.Context.crack_width
        for the arrays.

        The plane comes from the keyframe's geometry map, and an index shard sees only its own points, so world > 1 raises
        ValueError.  (The shards' key images would have to be merged first, as for geometry_maps; not built.)"""
        if self.world > 1:
            raise ValueError("crack_width: an index shard sees only its own points; the per-pixel keys of the shards would "
                             "have to be merged across ranks (all-reduce MIN), which is not built: run it on one rank "
                             "holding the whole map")
        return self.engine.ctx.crack_width(frame, threshold, plane_radius, want)

    def crack_map(self, frames=None, threshold: int = 0, plane_radius: int = 150, min_views: int = 1, link_radius: float = 0.02,
                  lengths: bool = False, skeleton: bool = False, skeleton_step=None, directions: bool = False, up=(0.0, 0.0, 1.0),
                  branches: bool = False, prune=None) -> dict:
        """The crack widths of the keyframes brought back to the map, and the map's cracks ("Crack widths on the
        map"): begin, one add per keyframe of `frames` (None: all of them), the components, end.  dict of the per-point arrays of
        capi.Context.crack_fuse_fetch (width_mean, width_best, best_frame, views, seen, centres, min_q, max_q, sum_q) and of
        capi.Context.crack_components (label, ids, stats, box, crack_points, components), plus contributors and credited
        (per added keyframe).  This is what compute_skeleton_edge_pts of scripts/genNormAndDistanceMask.py leaves as one
        record per hand-picked pixel, for every map point and with the cracks told apart.

        lengths: the dict gains `lengths`, the dict of capi.Context.crack_lengths for the same min_views and link_radius
        ("Crack lengths on the map"): per crack a geodesic length, its ends and an ordered polyline, per point
        its arc position.  Off, the return value is what it was.

        skeleton: the dict gains `skeleton`, the dict of capi.Context.crack_skeleton for the same min_views and link_radius and
        the band width skeleton_step (metres; None: 2 * link_radius) ("Crack skeletons on the map"): per crack its
        nodes, edges, ends, junctions, loops and skeleton length.  Off, the return value is what it was.

        directions: the dict gains `directions`, the dict of capi.Context.crack_directions for the same min_views and
        link_radius ("Crack directions on the map"): per point the tangent of its crack and its anisotropy, per
        crack the axis, plus inclination_deg = acos|axis . up| (0..90) and cls (vertical below 22.5, horizontal above 67.5, else
        diagonal; none without an axis) against the vertical `up` (finite, not zero).  Off, the return value is what it was.

        branches: the dict gains `branches`, the dict of capi.Context.crack_branches for the same min_views, link_radius and
        skeleton_step and the bound `prune` (metres; None: twice the band width) ("Crack branches on the map"): the
        cracks arm by arm, short spurs pruned, per branch its points, widths, length and axis.  Off, the return value is what it
        was.

        An index shard sees only its own points, so world > 1 raises ValueError.  (The shards' key images would have to be
        merged first, as for geometry_maps; not built.)"""
        if self.world > 1:
            raise ValueError("crack_map: an index shard sees only its own points; the per-pixel keys of the shards would "
                             "have to be merged across ranks (all-reduce MIN), which is not built: run it on one rank "
                             "holding the whole map")
        up = np.asarray(up, np.float64).reshape(-1)
        if directions and not (up.shape == (3,) and np.isfinite(up).all() and np.linalg.norm(up) > 0.0):
            raise ValueError("crack_map: up must be three finite numbers, not all zero")
        ctx = self.engine.ctx
        frames = range(ctx.n_frames) if frames is None else frames
        ctx.crack_fuse_begin()
        try:
            counts = [ctx.crack_fuse_add(int(f), threshold, plane_radius) for f in frames]
            out = ctx.crack_fuse_fetch()
            out.update(ctx.crack_components(min_views, link_radius))
            if directions:  # (it leaves the same component table)
                d = ctx.crack_directions(min_views, link_radius)
                has = d["axis"].any(axis=1)
                incl = np.degrees(np.arccos(np.minimum(1.0, np.abs(d["axis"] @ (up / np.linalg.norm(up))))))
                d["inclination_deg"] = np.where(has, incl, 0.0)
                d["cls"] = ["none" if not h else "vertical" if a < 22.5 else "horizontal" if a > 67.5 else "diagonal"
                            for h, a in zip(has.tolist(), incl.tolist())]
                out["directions"] = d
            if lengths:
                out["lengths"] = ctx.crack_lengths(min_views, link_radius)
            if skeleton:
                out["skeleton"] = ctx.crack_skeleton(min_views, link_radius, skeleton_step)
            if branches:  # (it leaves the same skeleton, length and component tables)
                step = capi.crack_skeleton_step(link_radius) if skeleton_step is None else skeleton_step
                out["branches"] = ctx.crack_branches(min_views, link_radius, step, 2.0 * step if prune is None else prune)
            out["contributors"] = [c[0] for c in counts]
            out["credited"] = [c[1] for c in counts]
            self.last_crack_map = dict(width_mean=out["width_mean"], label=out["label"])  # (ortho_map draws them)
            return out
        finally:
            ctx.crack_fuse_end()

    def run(self, download: bool = True, local_smooth_radius: float = 0.0, fuse_labels: bool = False, output_leaf: float = 0.0):
        """Local points' colours: dict(rgb (n,3) uint8, has (n,) uint8).

        output_leaf > 0: the dict gains `voxel` -- dict(xyz (m,3) float32, rgb (m,3) uint8, count (m,) uint32, rows, and label
        (m,) uint8 with fuse_labels): one row per occupied voxel of that edge over the coloured points, reduced on the device
        (what pcl::VoxelGrid at that leaf makes of the output files; DESIGN.md, "Voxel-grid output").  It reads the colours
        as they are after the local smoothing.  With download=False only these rows leave the device.  The sums are local to
        a rank and their exchange is not built: world > 1 raises ValueError.

        fuse_labels: one segmentation label per point from the masks of its top-5 views ("Fused segmentation
        labels"); the dict gains label, hits, views (n,) uint8 (rank-local, as the colours; without download they stay on
        the device: engine.ctx.colour_labels_device()).  Every keyframe needs an uploaded mask.  The local colour
        smoothing leaves them alone.

        Multi-rank: the keyframes are split into `chunks` groups (0 = chosen from the size of the maps); the
        all-reduce(MIN) of one group's depth maps (RCCL stream) overlaps the depth pass of the next group.
        local_smooth_radius > 0: smoothColorsWithLocalRegion over the finished colours (one rank only; the reference
        leaves it off, PointCloudProcessor.cpp:597).
        capi.MATCH_RADIUS needs the whole map on one rank: with world > 1 it raises ValueError."""
        if self.world > 1 and getattr(self.engine, "match_mode", None) == capi.MATCH_RADIUS:
            raise ValueError("match_mode MATCH_RADIUS: a map point takes samples from its neighbours, which other ranks "
                             "hold; run it on one rank holding the whole map")
        if local_smooth_radius and self.world > 1:
            raise ValueError("local_smooth_radius: the local colour smoothing runs on one rank holding the whole map "
                             "(smooth the gathered words with Context.colour_smooth_local_packed)")
        if output_leaf and self.world > 1:
            raise ValueError("output_leaf: the voxel sums of the index shards would have to be added across ranks, which is not "
                             "built; run it on one rank holding the whole map")
        if fuse_labels != getattr(self.engine, "fuse_labels", False):
            self.engine.set_label_fusion(fuse_labels)
        if self.world == 1:
            self.engine.depth_pass()
            if self.balance_exposure:
                out = self._colour_balanced(download)
            else:
                out = self.engine.colour_from_depth(download=download)
            if local_smooth_radius:
                out = self.engine.smooth_colours_local(local_smooth_radius, download=download)
            out = self._with_labels(out, fuse_labels, download)
            if output_leaf:
                out = dict(out, voxel=self._voxel_output(output_leaf, fuse_labels))
            return out
        import torch.distributed as dist

        F = self.engine.n_frames
        t = self.engine.depth_maps_tensor()
        cells = t.numel() // max(F, 1)
        # chunks = 0: one all-reduce for small maps (splitting the depth pass costs ~0.1 ms per extra chunk at C3,
        # more than overlapping a ~10 MB all-reduce saves), two keyframe groups from 32 MB of maps up
        chunks = self.chunks if self.chunks > 0 else (1 if t.numel() * 4 < (32 << 20) else 2)
        # group boundaries on multiples of 32 keyframes (whole tile-mask words) when there are enough keyframes
        align = 32 if F >= 64 * chunks else 1
        bounds = sorted({min(F, ((F * c) // chunks + align - 1) // align * align) for c in range(chunks)} | {0, F})
        works = []
        for f0, f1 in zip(bounds[:-1], bounds[1:]):
            self.engine.depth_pass(f0, f1)
            if not getattr(self.engine, "_on_torch_stream", False) and t.is_cuda:
                self.engine.ctx.synchronize()
            # ranges are positive finite floats: float MIN == the uint-bits MIN the kernel used
            works.append(dist.all_reduce(t[f0 * cells:f1 * cells], op=dist.ReduceOp.MIN, group=self.group, async_op=True))
        for w in works:
            w.wait()  # stream-level wait on GPUs, blocking on gloo
        if t.is_cuda and not getattr(self.engine, "_on_torch_stream", False):
            import torch

            torch.cuda.current_stream().synchronize()
        return self._with_labels(self.engine.colour_from_depth(download=download), fuse_labels, download)

    def _colour_balanced(self, download: bool):
        """The staged colour stage (the depth maps are there): colour pass over all keyframes, pair statistics, gains, gained
        finalise.  The gains are cleared again afterwards, so the engine's one-shot calls keep working."""
        ctx = self.engine.ctx
        ctx.colour_reset()
        ctx.colour_pass()
        n, s = ctx.view_pair_stats()
        self.gains = capi.exposure_gains(n, s, *self.exposure_sigma)
        ctx.set_frame_gains(self.gains)
        try:
            out = ctx.colour_finalise(download=download)
        finally:
            ctx.set_frame_gains(None)
        return dict(rgb=out["rgb"], has=out["has"])

    def gather(self, local: dict, n_total: int):
        """All-gather the per-shard colours (and the fused labels, when `local` holds them) into full-length arrays
        (every rank)."""
        if self.world == 1:
            return local
        import torch
        import torch.distributed as dist

        sizes = [shard_bounds(n_total, r, self.world) for r in range(self.world)]
        maxn = max(hi - lo for lo, hi in sizes)
        extra = [k for k in ("label", "hits", "views") if local.get(k) is not None]
        packed = np.zeros((maxn, 4 + len(extra)), np.uint8)
        lo, hi = sizes[self.rank]
        packed[: hi - lo, :3] = local["rgb"]
        packed[: hi - lo, 3] = local["has"]
        for c, k in enumerate(extra):
            packed[: hi - lo, 4 + c] = local[k]
        dev = "cuda" if dist.get_backend(self.group) == "nccl" else "cpu"
        mine = torch.from_numpy(packed).to(dev)
        outs = [torch.empty_like(mine) for _ in range(self.world)]
        dist.all_gather(outs, mine, group=self.group)
        rgb = np.zeros((n_total, 3), np.uint8)
        has = np.zeros(n_total, np.uint8)
        more = {k: np.zeros(n_total, np.uint8) for k in extra}
        for r, (lo, hi) in enumerate(sizes):
            a = outs[r].cpu().numpy()
            rgb[lo:hi] = a[: hi - lo, :3]
            has[lo:hi] = a[: hi - lo, 3]
            for c, k in enumerate(extra):
                more[k][lo:hi] = a[: hi - lo, 4 + c]
        return dict(rgb=rgb, has=has, **more)


def _rows_xyz(who: str, xyz, n: int | None = None):
    """the map an "auto" orthographic frame is fitted to, as (rows, 3) float32: given as that, or as (x, y, z)"""
    import numpy as np

    if xyz is None:
        raise ValueError(f"{who}: frame \"auto\" is fitted to the map: pass it as xyz (or pass a frame dict)")
    if isinstance(xyz, (tuple, list)) and len(xyz) == 3 and np.ndim(xyz[0]) == 1:
        xyz = np.stack([np.asarray(a, np.float32) for a in xyz], axis=1)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if n is not None and len(xyz) != n:
        raise ValueError(f"{who}: xyz has {len(xyz)} rows, the uploaded cloud {n}")
    return xyz


def ortho_texture_request(who: str, texture: dict | None) -> dict | None:
    """the keyword arguments of capi.Context.ortho_texture from a texture=dict(scale[, views, interpolate, max_step])"""
    if texture is None:
        return None
    unknown = set(texture) - {"scale", "views", "interpolate", "max_step"}
    if unknown or "scale" not in texture:
        raise ValueError(f"{who}: texture is dict(scale[, views, interpolate, max_step]), got {sorted(texture)}")
    return dict(scale=int(texture["scale"]), views=int(texture.get("views", 1)), interpolate=bool(texture.get("interpolate", True)),
                max_step=float(texture.get("max_step", 0.05)))


def ortho_defects_request(who: str, defects: dict | None) -> dict | None:
    """the keyword arguments of capi.Context.ortho_defects from a defects=dict(threshold[, window, refine, min_support,
    min_pixels, classes])"""
    if defects is None:
        return None
    known = ("threshold", "window", "refine", "min_support", "min_pixels", "classes")
    extra = sorted(set(defects) - set(known))
    if extra or "threshold" not in defects:
        raise ValueError(f"{who}: defects is dict(threshold[, window, refine, min_support, min_pixels, classes]); got {sorted(defects)}")
    return {k: defects[k] for k in known if k in defects}


def ortho_defect_layers(ctx, request: dict, gsd: float, facet: int | None = None) -> dict:
    """defect_dev / defect_class / defect_region and the list `defects` of the live, finished map of `ctx` (capi.Context
    .ortho_defects, _fetch, _table): the library's integers, and per region the metres derived from them on the host"""
    counts = ctx.ortho_defects(**request)
    layers = ctx.ortho_defects_fetch()
    rows = ctx.ortho_defects_table()
    width = layers["dev"].shape[1]
    quantum, g2 = 2.0 ** -20, float(gsd) * float(gsd)
    found = []
    for r in rows:
        d = dict(zip(capi.DEFECT_ROW, (int(v) for v in r)))
        item = dict(kind="hollow" if d["class"] == capi.DEFECT_HOLLOW else "bulge", pixels=d["pixels"], area_m2=d["pixels"] * g2,
                    volume_m3=d["sum_dev"] * quantum * g2, depth_m=d["max_dev"] * quantum,
                    depth_px=(d["max_pixel"] % width, d["max_pixel"] // width), box_px=(d["col_min"], d["row_min"], d["col_max"], d["row_max"]),
                    centroid_px=(d["sum_col"] / d["pixels"], d["sum_row"] / d["pixels"]), measured_fraction=d["measured"] / d["pixels"],
                    open_pixels=d["open"], first_pass_pixels=d["first_pass"], row=[int(v) for v in r])
        if facet is not None:
            item["facet"] = int(facet)
        found.append(item)
    return dict(defect_dev=layers["dev"], defect_class=layers["cls"], defect_region=layers["region"], defects=found, defect_counts=counts)


def ortho_crack_layers(index, map_width, map_crack) -> dict:
    """width (H, W) float32 and crack (H, W) int32 of an orthographic map from its index layer and the per-point arrays of the
    crack chain on the map: map_width[index] and map_crack[index], 0 and -1 on empty pixels."""
    import numpy as np

    empty = index == np.uint32(0xFFFFFFFF)
    at = np.where(empty, 0, index).astype(np.int64)
    return dict(width=np.where(empty, np.float32(0), np.asarray(map_width, np.float32)[at]).astype(np.float32),
                crack=np.where(empty, -1, np.asarray(map_crack, np.int32)[at]).astype(np.int32))


def ortho_change_layers(index, distance, status) -> dict:
    """change (H, W) float32 and change_status (H, W) uint8 of an orthographic map from its index layer and the per-point arrays
    of the map comparison: distance[index] and status[index], 0 on empty pixels."""
    import numpy as np

    empty = index == np.uint32(0xFFFFFFFF)
    at = np.where(empty, 0, index).astype(np.int64)
    return dict(change=np.where(empty, np.float32(0), np.asarray(distance, np.float32)[at]).astype(np.float32),
                change_status=np.where(empty, 0, np.asarray(status, np.uint8)[at]).astype(np.uint8))


def keyframe_block(n_frames: int, rank: int, world: int):
    """[f0, f1): the keyframes whose hulls rank `rank` takes when hidden_points_removal runs over `world` GPUs."""
    return n_frames * rank // world, n_frames * (rank + 1) // world


class HullSharding:
    """hidden_points_removal (view_culling.cpp:266-334) over point-index shards.  A keyframe's hull is taken over EVERY
    candidate of the map, so an index shard cannot decide its own points: every rank holds a second context with the whole
    map (`hull_ctx`, cull_mode PCP_CULL_HPR, no images), takes the hulls of its block of keyframes there in one
    pcp_depth_pass (several keyframes in flight), and the verdicts -- one flag per map point -- go to the ranks that own the
    points: in round i rank o holds keyframe f0(o) + i and sends every rank k the slice [lo(k), hi(k)) of its verdicts, ONE
    BIT per point, in one all_to_all_single (a rank receives W slices of its own index range: ~n / 8 bytes per round and
    rank where an all-gather of byte flags moved W x n to everyone; host/pcp_multi.hpp sends slices the same way).  Every
    rank imports the slices into its shard context (`shard_ctx`, PCP_DEPTH_BATCHED), which then colours / dumps from the
    bits exactly as a one-GPU run does.  With the "nccl" backend the flags stay in device memory from pcp_cull_frame to
    pcp_hull_flags_import (ABI v5)."""

    def __init__(self, hull_ctx, shard_ctx, n_total: int, rank: int, world: int, group=None):
        self.hull_ctx, self.shard_ctx = hull_ctx, shard_ctx
        self.n_total, self.rank, self.world, self.group = int(n_total), rank, world, group

    @staticmethod
    def packed_bytes(count: int) -> int:
        """bytes of a bit-packed slice of `count` verdicts (bit j of byte b = point 8 b + j of the slice)"""
        return (int(count) + 7) // 8

    def run(self, n_frames: int, device: str | None = None):
        """Returns dict(hull_s, exchange_s, kept, exchange_bytes, rounds) -- kept = hull vertices of this rank's keyframes,
        exchange_bytes = what this rank sent (== what it received up to padding) over all rounds."""
        import time

        import torch
        import torch.distributed as dist

        W, r, n = self.world, self.rank, self.n_total
        bounds = [shard_bounds(n, k, W) for k in range(W)]
        lo, hi = bounds[r]
        mine_n = hi - lo
        f0, f1 = keyframe_block(n_frames, r, W)
        t0 = time.perf_counter()
        if f1 > f0:
            self.hull_ctx.depth_pass(f0, f1)
        self.hull_ctx.synchronize()
        t_hull = time.perf_counter() - t0
        on_gpu = W > 1 and dist.get_backend(self.group) == "nccl"
        dev = (device or "cuda") if on_gpu else "cpu"
        blocks = [keyframe_block(n_frames, k, W) for k in range(W)]
        rounds = max(b1 - b0 for b0, b1 in blocks)
        send_sizes = [self.packed_bytes(b - a) for a, b in bounds]      # to rank k: its index range, bit-packed
        recv_sizes = [self.packed_bytes(mine_n)] * W                    # from every rank: my index range
        flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        padded = torch.zeros(8 * max(send_sizes), dtype=torch.uint8, device=dev)  # a slice, zero-padded to whole bytes
        weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
        shifts = torch.arange(8, dtype=torch.uint8, device=dev)
        send = torch.zeros(sum(send_sizes), dtype=torch.uint8, device=dev)
        recv = torch.zeros(sum(recv_sizes), dtype=torch.uint8, device=dev)
        kept = moved = 0
        t0 = time.perf_counter()
        for i in range(rounds):
            f = f0 + i
            if f < f1:
                if on_gpu:
                    kept += self.hull_ctx.cull_frame_into(f, flags.data_ptr())  # from the whole-run bits: nothing recomputed
                else:
                    keep, _, k = self.hull_ctx.cull_frame(f)
                    flags.copy_(torch.from_numpy(np.ascontiguousarray(keep)))
                    kept += int(k)
                at = 0
                for (a, b), sz in zip(bounds, send_sizes):
                    padded.zero_()
                    padded[: b - a] = flags[a:b] != 0
                    send[at:at + sz] = (padded[: 8 * sz].view(sz, 8) * weights).sum(dim=1, dtype=torch.uint8)
                    at += sz
            else:
                send.zero_()  # (no keyframe of mine in this round: the others ignore what arrives from me)
            if W > 1:
                dist.all_to_all_single(recv, send, output_split_sizes=recv_sizes, input_split_sizes=send_sizes, group=self.group)
                moved += int(send.numel())
            else:
                recv.copy_(send)
            psz = recv_sizes[0]
            for k in range(W):
                fk0, fk1 = blocks[k]
                if fk0 + i >= fk1:
                    continue
                bits = ((recv[k * psz:(k + 1) * psz].unsqueeze(1) >> shifts) & 1).reshape(-1)[:mine_n].contiguous()
                if on_gpu:
                    torch.cuda.current_stream().synchronize()  # the library imports on its own stream
                    self.shard_ctx.hull_flags_import_ptr(fk0 + i, bits.data_ptr())
                    self.shard_ctx.synchronize()  # `bits` is released next
                else:
                    self.shard_ctx.hull_flags_import(fk0 + i, bits.cpu().numpy())
        if on_gpu:
            self.shard_ctx.synchronize()
        return dict(hull_s=t_hull, exchange_s=time.perf_counter() - t0, kept=kept, exchange_bytes=moved, rounds=rounds)


class VisualLiDARCalibration:
    """vlcal::VisualLiDARCalibration::calibrate (calibrate.cpp:42-126) over an index-sharded map.

    A keyframe's joint histogram is a sum over its points: every rank accumulates the histograms of its shard, the ranks
    add them (all-reduce SUM, 8 B x F x (7 bins^2 + bins): 0.9 MB at 64 keyframes) and turn the sums into cost and
    gradient -- identical numbers everywhere, so the BFGS loops of all ranks walk in lockstep without a broadcast.  The
    shards' single-keyframe culls need the MIN-merged depth maps (PointCloudColorizer.run or depth pass + all-reduce
    first, then ctx.set_depth_source(True))."""

    def __init__(self, engine: HipEngine, rank: int = 0, world: int = 1, group=None):
        self.engine = engine
        self.rank = rank
        self.world = world
        self.group = group

    def prepare(self) -> int:
        return self.engine.ctx.nid_prepare()

    def _hist_tensor(self):
        import torch

        ptr, n = self.engine.ctx.nid_histograms_device()
        return torch.as_tensor(_DeviceArray(ptr, n, "<f8"), device=f"cuda:{self.engine.device}")

    def evaluate(self, T, bins: int = 16):
        ctx = self.engine.ctx
        ctx.nid_accumulate(T, bins)
        if self.world > 1:
            import torch.distributed as dist

            ctx.synchronize()
            t = self._hist_tensor()
            if dist.get_backend(self.group) == "nccl":
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
                import torch

                torch.cuda.current_stream().synchronize()
            else:  # gloo rehearsal: through the host
                h = t.cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
                t.copy_(h)
                import torch

                torch.cuda.synchronize()
        cost, grad, ok = ctx.nid_finish(bins)
        if self.world > 1:
            # every rank derives (cost, gradient) from the same summed histograms, so every rank's optimiser takes the
            # same steps without a broadcast -- IF the all-reduce hands every rank the same bits.  Checked instead of
            # assumed: a rank that saw different numbers would walk a different line search and the ranks would wait
            # for each other in different collectives for ever.
            import torch
            import torch.distributed as dist

            mine = torch.tensor([cost, *[float(g) for g in grad], float(ok)], dtype=torch.float64).view(torch.int64)  # bit patterns: NaN == NaN
            lo, hi = mine.clone(), mine.clone()
            if dist.get_backend(self.group) == "nccl":
                lo, hi = lo.cuda(), hi.cuda()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.group)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.group)
            if not torch.equal(lo.cpu(), hi.cpu()):
                raise RuntimeError("NID cost / gradient differ between the ranks after the all-reduce of the histograms: "
                                   f"min {lo.tolist()} max {hi.tolist()}")
        return cost, grad, ok

    def calibrate(self, T_init=None, bins: int = 16, max_outer_iterations: int = 10):
        """T_camera_lidar_optimized (4x4), final cost, evaluations -- identity initial guess as calibrate.cpp:45-51"""
        Ti = np.eye(4) if T_init is None else np.asarray(T_init, np.float64)
        if self.world == 1:
            return self.engine.ctx.nid_optimize(Ti, bins, max_outer_iterations)
        return self.engine.ctx.nid_optimize_with(self.evaluate, Ti, bins, max_outer_iterations)


class CloudSmooth:
    """CloudSmooth::process: MovingLeastSquares (+ optional SOR brackets).
    local_plane=(radius, step): SAMPLE_LOCAL_PLANE's disk (MLSParameters slp_upsampling_radius / _stepsize), applied to
    the context before every run; None leaves the context's setting (the reference's 0.05 / 0.01 unless changed)."""

    def __init__(self, engine: HipEngine, params: capi.MLSParams | None = None, local_plane: tuple[float, float] | None = None):
        self.engine = engine
        self.params = params if params is not None else capi.default_mls_params()
        self.local_plane = local_plane

    def _apply_local_plane(self):
        if getattr(self, "local_plane", None) is not None:
            self.engine.ctx.set_mls_local_plane(*self.local_plane)

    def process_sharded(self, n_total: int, rank: int, world: int, group=None):
        """MLS (upsampling NONE) with the queries dealt out over `world` ranks by slabs of the stage's own spatial order
        (whole wavefronts: 1 / world of the work whatever order the caller's points come in): every rank holds the whole
        cloud, fits its slab, the variable-length results are all-gathered and merged by source index.
        Returns the full result, in input order, on every rank."""
        if getattr(self.params, "upsampling", None) == capi.UPSAMPLING_SAMPLE_LOCAL_PLANE:
            raise ValueError("process_sharded: SAMPLE_LOCAL_PLANE is not sharded (each disk follows the sign of its point's "
                             "fitted normal, which a re-ordered fit may flip); run process() on one GPU")
        ctx = self.engine.ctx
        local = ctx.mls_fetch(ctx.mls_process_slab(self.params, rank, world))
        if world == 1:
            return local
        import torch
        import torch.distributed as dist

        dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        m = torch.tensor([len(local["index"])], dtype=torch.int64, device=dev)
        counts = [torch.zeros_like(m) for _ in range(world)]
        dist.all_gather(counts, m, group=group)
        counts = [int(c.item()) for c in counts]
        cap = max(max(counts), 1)
        packed = np.zeros((cap, 8), np.float32)  # xyz(3) normal(3) curvature index(as int bits)
        k = len(local["index"])
        packed[:k, 0:3] = local["xyz"]
        packed[:k, 3:6] = local["normal"]
        packed[:k, 6] = local["curvature"]
        packed[:k, 7] = local["index"].view(np.float32)
        mine = torch.from_numpy(packed).to(dev)
        outs = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(outs, mine, group=group)
        parts = [outs[r].cpu().numpy()[: counts[r]] for r in range(world)]
        allp = np.concatenate(parts, axis=0) if parts else np.zeros((0, 8), np.float32)
        idx = np.ascontiguousarray(allp[:, 7]).view(np.int32)
        allp = allp[np.argsort(idx, kind="stable")]  # a point is fitted by exactly one slab: the merge restores input order
        return dict(xyz=np.ascontiguousarray(allp[:, 0:3]), normal=np.ascontiguousarray(allp[:, 3:6]),
                    curvature=np.ascontiguousarray(allp[:, 6]), index=np.ascontiguousarray(allp[:, 7]).view(np.int32))

    def outlier_removal_sharded(self, n_total: int, rank: int, world: int, group=None):
        """StatisticalOutlierRemoval (cloudSmooth.cpp:109-116) with the queries dealt out by slabs of the filter's own spatial
        order: every rank holds the whole cloud, computes the mean distances and per-chunk (sum, sum of squares) of its
        slab, the chunk sums are put together (ceil(n / 16384) pairs of doubles), every rank classifies its slab and the
        keep flags are combined.  Equal to ctx.sor() on one GPU bit for bit.  Returns the full keep mask."""
        ctx = self.engine.ctx
        c = ctx.sor_chunk_points()
        chunks = (n_total + c - 1) // c
        sums = np.zeros((chunks, 2), np.float64)
        first, mine = ctx.sor_partial(self.params.sor_mean_k, rank, world)
        sums[first:first + len(mine)] = mine
        if world > 1:
            import torch
            import torch.distributed as dist

            dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
            # every chunk is owned by exactly one rank and zero elsewhere: x + 0.0 is exact, the sum IS the concatenation
            t = torch.from_numpy(sums).to(dev)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            sums = t.cpu().numpy()
        keep = ctx.sor_finish(self.params.sor_std_mul, sums, rank, world)[0]
        if world > 1:
            t = torch.from_numpy(keep).to(dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            keep = t.cpu().numpy()
        return keep

    def process(self, with_outlier_removal: bool = True):
        """SOR -> MLS (+ upsampling) -> SOR as cloudSmooth.cpp:109-164; MLS alone when asked.  An upsampled cloud that one
        result cannot hold (the reference's VOXEL_GRID_DILATION 1 mm x 4 on a real map) goes through the streamed form and is
        gathered on the host, as the C++ shim does (host/pcp_shim.hpp)."""
        ctx = self.engine.ctx
        self._apply_local_plane()
        if not with_outlier_removal:
            return ctx.mls_fetch(ctx.mls_process(self.params))
        try:
            return ctx.mls_fetch(ctx.cloud_smooth(self.params))
        except capi.PcpError as e:
            if e.code != capi.PCP_ERR_NOMEM or self.params.upsampling != 3:
                raise
        # (one cloud is what the caller asked for: fine as long as a later upload can take it)
        parts = list(self.process_streamed(1 << 28, max_rows=MAX_UPLOAD_POINTS))
        if not parts:
            return ctx.mls_fetch(0)
        import numpy as np

        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}

    def process_streamed(self, chunk_capacity: int = 1 << 28, hold_device_memory: bool = False, max_rows: int | None = None):
        """The whole CloudSmooth::process through pcp_cloud_smooth_stream_*: yields the survivors of the trailing outlier removal
        chunk by chunk (dicts as mls_fetch returns them), in the order the one-shot form returns them; `self.streamed` holds
        (rows before the last filter, rows kept, chunks) and the stream's diagnostics.  max_rows: a caller that gathers the
        chunks into one cloud passes the most it can use; more kept rows raise before the first chunk is fetched."""
        ctx = self.engine.ctx
        total, kept, chunks = ctx.cloud_smooth_stream_begin(self.params, chunk_capacity)
        self.streamed = {"rows": total, "kept": kept, "chunks": chunks, **ctx.cloud_smooth_stream_stats()}
        if max_rows is not None and kept > max_rows:
            ctx.cloud_smooth_stream_end()
            raise ValueError(f"the smoothed cloud has {kept} rows, more than one upload takes ({max_rows}): it cannot be gathered "
                             "for the colour stage; colour it chunk by chunk (process_and_colourise_streamed, --streamColour 1 on "
                             "the command line)")
        try:
            while True:
                m = ctx.cloud_smooth_stream_next()
                if m == 0:
                    break
                yield ctx.mls_fetch(m)
        finally:
            if not hold_device_memory:
                ctx.cloud_smooth_stream_end()

    def process_and_colourise_streamed(self, colour_engine: HipEngine, chunk_capacity: int = 1 << 28, fuse_labels: bool = False,
                                       on_smoothed=None, download: bool = True, output_leaf: float = 0.0, ortho: dict | None = None):
        """CloudSmooth::process followed by the colourisation of the smoothed cloud (PointCloudProcessor.cpp:139-145, 474-602)
        for clouds whose smoothed rows exceed one upload: the mirror of the C++ shim's processAndColorizeStreamed.  A chunk of
        the chain's voxel order is an index shard in time -- the depth maps are a MIN over all points and a point's colour
        depends only on its own projection, the merged maps and the images -- so the chunks' results concatenate to the
        one-shot result bit for bit ("Streamed colourisation").

        `colour_engine`: a second HipEngine on the same GPU with camera, keyframes and images (masks for fuse_labels) set;
        every chunk reaches it device to device (pcp_upload_cloud_from_result).
          sweep A  every chunk: depth pass over all keyframes, merged into the accumulator; on_smoothed(rows) -- the dict
                   mls_fetch returns -- is called per chunk when given (the <stem>_mls.pcd rows);
          sweep B  the stream rewound: depth pass (tile masks), the accumulator applied, colours, compaction on the device.
        Yields one dict per chunk with a coloured row: index (the source index the chain reports), xyz, rgb and, with
        fuse_labels, label.  download=False: the rows stay on the device and every dict holds only `count`, the chunk's
        coloured rows (what the device work alone costs).  `self.streamed_colour` holds chunks, rows, coloured and the seconds
        of both sweeps.

        output_leaf > 0: the coloured rows of every chunk are also reduced on the device to one row per occupied voxel of
        that edge ("Voxel-grid output"): an accumulation begins before sweep B, takes every chunk after it is
        coloured and is finished after the sweep; `self.voxel_output` then holds dict(xyz, rgb, count[, label]) and
        `self.streamed_colour` gains voxel_add_s, voxel_finish_s and the accumulator's stats.  With download=False these rows
        are all that leaves the device.

        ortho: dict(frame, gsd, fill_radius[, xyz, viewer, texture]) -- one orthographic map of all the coloured rows (DESIGN.md,
        "Orthographic maps"): the frame is resolved and the map begun on `colour_engine` before any other work (a bad frame or
        a gsd too fine for the extent is refused at once), every chunk is added after it is coloured under index_base = the
        rows of the chunks before it (the row's place in the concatenated smoothed cloud), the map is finished and fetched
        after sweep B; `self.ortho_output` then holds the layers, the frame and the counts, and `self.streamed_colour` gains
        ortho_add_s and ortho_finish_s.  frame "auto" (the default): fitted on the host to `xyz`, the raw map the caller
        uploaded to this engine ((n, 3) or (x, y, z)) -- the same surface up to the chain's dilation -- seen from the side
        of `viewer` (3 numbers, e.g. the mean keyframe position).  Works with download=False: the map is then, with the voxel
        rows, all that leaves.  texture: dict(scale[, views, interpolate, max_step]) -- `self.ortho_output` gains photo, the
        orthophoto of the finished map ("Orthophotos"), textured after the last chunk on the merged depth maps
        (None when no chunk held a row)."""
        ctx, col = self.engine.ctx, colour_engine.ctx
        ortho_texture_request("ortho", None if ortho is None else ortho.get("texture"))  # (a bad request is refused before any work)
        if ortho is not None:
            frame = ortho.get("frame", "auto")
            if isinstance(frame, str):
                if frame != "auto":
                    raise ValueError(f"ortho: frame {frame!r} is neither a dict nor \"auto\"")
                frame = capi.ortho_fit_frame_host(_rows_xyz("ortho", ortho.get("xyz")), ortho.get("gsd", 0.01), viewer=ortho.get("viewer"))
            col.ortho_begin(frame)  # (the map outlives the chunks' uploads; ended below whatever happens)
        try:
            yield from self._streamed_sweeps(colour_engine, chunk_capacity, fuse_labels, on_smoothed, download, output_leaf,
                                             ortho, frame if ortho is not None else None)
        finally:
            if ortho is not None:
                col.ortho_end()

    def _streamed_sweeps(self, colour_engine, chunk_capacity, fuse_labels, on_smoothed, download, output_leaf, ortho, frame):
        """the two sweeps of process_and_colourise_streamed; `frame`: of the orthographic map begun on colour_engine"""
        import time

        ctx, col = self.engine.ctx, colour_engine.ctx
        self._apply_local_plane()
        col.set_label_fusion(fuse_labels)
        col.depth_accum_reset()
        total, kept, chunks = ctx.cloud_smooth_stream_begin(self.params, chunk_capacity)
        self.streamed = {"rows": total, "kept": kept, "chunks": chunks, **ctx.cloud_smooth_stream_stats()}
        stats = self.streamed_colour = {"chunks": chunks, "rows": 0, "coloured": 0, "sweep_a_s": 0.0, "sweep_b_s": 0.0}
        try:
            t0 = time.perf_counter()
            for _ in range(chunks):  # (chunks without rows are skipped by _next: the calls left over return 0)
                m = ctx.cloud_smooth_stream_next()
                if m == 0:
                    continue
                stats["rows"] += m
                col.upload_cloud_from_result(ctx)
                col.depth_pass()
                col.depth_accum_merge()
                if on_smoothed is not None:
                    on_smoothed(ctx.mls_fetch(m))
            col.synchronize()
            stats["sweep_a_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            self.voxel_output = self.ortho_output = None
            if ortho is not None:
                stats["ortho_add_s"] = 0.0
                rows_before = 0
            if output_leaf:
                col.voxel_reduce_begin(output_leaf)
                stats["voxel_add_s"] = 0.0
                stats["voxel_add_chunk_s"] = []
            ctx.cloud_smooth_stream_seek(0)
            for _ in range(chunks):
                m = ctx.cloud_smooth_stream_next()
                if m == 0:
                    continue
                col.upload_cloud_from_result(ctx)
                col.depth_pass()  # builds this chunk's tile masks, as on a shard before the all-reduce(MIN)
                col.depth_accum_apply()
                col.colorize_from_depth(download=False)
                if output_leaf:
                    col.synchronize()  # (the colour pass is asynchronous: the clock below takes the add alone)
                    t1 = time.perf_counter()
                    col.voxel_reduce_add()
                    stats["voxel_add_chunk_s"].append(time.perf_counter() - t1)
                    stats["voxel_add_s"] += stats["voxel_add_chunk_s"][-1]
                if ortho is not None:
                    col.synchronize()
                    t1 = time.perf_counter()
                    col.ortho_add(rows_before)
                    stats["ortho_add_s"] += time.perf_counter() - t1
                    rows_before += m
                out = col.colour_compact(capacity=None if download else 0, want_label=fuse_labels and download)
                count = out.pop("count")
                stats["coloured"] += count
                stats["sweep_b_s"] = time.perf_counter() - t0
                if count and not download:
                    yield {"count": count}
                elif count:
                    out["index"] = ctx.mls_fetch_index(m)[out["index"]]
                    yield out
            if output_leaf:
                t1 = time.perf_counter()
                col.voxel_reduce_finish()
                self.voxel_output = col.voxel_reduce_fetch(want_label=fuse_labels)
                stats["voxel_finish_s"] = time.perf_counter() - t1
                stats["voxel"] = col.voxel_reduce_stats()
            if ortho is not None:
                t1 = time.perf_counter()
                occupied, filled = col.ortho_finish(int(ortho.get("fill_radius", 0)))
                self.ortho_output = col.ortho_fetch(want_label=fuse_labels)
                stats["ortho_finish_s"] = time.perf_counter() - t1
                texture = ortho_texture_request("ortho", ortho.get("texture"))
                if texture is not None:  # (the colour engine holds the last chunk's cloud under the merged maps)
                    t1 = time.perf_counter()
                    self.ortho_output["photo"] = col.ortho_texture(**texture) if rows_before else None
                    stats["ortho_texture_s"] = time.perf_counter() - t1
                stats["ortho"] = col.ortho_stats()
                self.ortho_output.update(frame=capi.ortho_frame(frame).as_dict(), occupied=occupied, filled=filled,
                                         contributors=stats["ortho"]["contributors"])
            stats["sweep_b_s"] = time.perf_counter() - t0
        finally:
            if output_leaf:
                col.voxel_reduce_end()
            ctx.cloud_smooth_stream_end()
