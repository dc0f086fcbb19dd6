"""Streamed colourisation ("Streamed colourisation"): pcp_upload_cloud_from_result, the depth-map accumulator,
pcp_cloud_smooth_stream_seek, pcp_colour_compact and the pipeline generator built on them.  A chunk of the smoothing chain's
voxel order is an index shard in time, so every comparison against the one-shot forms is bit for bit."""
import numpy as np
import pytest

from conftest import cam_struct

pytestmark = pytest.mark.gpu

CHUNK = 4096  # voxels per chunk of the streamed chain (the smallest the chain takes)


def two_levels(seed=11):
    """two patches at different depths: the oblique keyframes see the near one in front of the far one, and the chain cuts
    along x, so the occluder and the occluded rows fall into different chunks"""
    rng = np.random.default_rng(seed)
    patch = lambda n, x0, x1, zc: np.stack([rng.uniform(x0, x1, n), rng.uniform(-1.1, -0.9, n), zc + rng.normal(0, 1e-3, n)], 1)  # noqa: E731
    pts = np.concatenate([patch(2500, 1.70, 1.95, 1.5), patch(3500, 2.00, 2.35, 1.9)]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    return pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()


def _levels_scene():
    from pointcloudprocessor_amd import synth

    cd = synth.camera_dict("tiny")
    W, H = cd["image_width"], cd["image_height"]
    th = np.arctan2(0.6, 1.0)
    q = (np.cos(th / 2), 0.0, np.sin(th / 2), 0.0)
    poses = np.array([(2, -1, -0.5, 1, 0, 0, 0), (1.2, -1, 0.5, *q), (1.35, -0.95, 0.40, *q), (2.05, -1.02, -0.2, 1, 0, 0, 0)],
                     np.float64)
    x, y, z = two_levels()
    return dict(cam=cd, x=x, y=y, z=z, poses=poses, images=[synth.make_image(f, W, H) for f in range(4)],
                masks=[synth.make_mask(f, W, H) for f in range(4)])


def _mls_params(capi):
    p = capi.default_mls_params()
    p.vgd_voxel_size = 0.003
    p.vgd_iterations = 1
    return p


def _views(ctx, capi, s, masks=False):
    """camera, keyframes and images of scene s on a context; its cloud is empty (the image uploads ask for one)"""
    ctx.set_camera(cam_struct(capi, s["cam"]))
    e = np.zeros(0, np.float32)
    ctx.upload_cloud(e, e, e)
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
        if masks:
            ctx.upload_mask(f, s["masks"][f])


def _packed(ctx):
    return ctx.download_result_packed()


# the levels scene smoothed and coloured in one shot: computed once, shared, never modified
_ONE_SHOT = {}


def _one_shot(gpu_ctx_factory):
    if not _ONE_SHOT:
        from pointcloudprocessor_amd import capi

        s = _levels_scene()
        a = gpu_ctx_factory()
        a.upload_cloud(s["x"], s["y"], s["z"])
        rows = a.mls_fetch(a.cloud_smooth(_mls_params(capi)))
        c = gpu_ctx_factory()
        _views(c, capi, s, masks=True)
        c.upload_cloud(rows["xyz"][:, 0], rows["xyz"][:, 1], rows["xyz"][:, 2])
        c.set_label_fusion(True)
        col = c.colorize()
        lab = c.colour_labels()
        _ONE_SHOT.update(scene=s, rows=rows, rgb=col["rgb"], has=col["has"], label=lab["label"], smooth_ctx=a, colour_ctx=c)
        for v in (rows["xyz"], rows["index"], col["rgb"], col["has"], lab["label"]):
            v.setflags(write=False)
    return _ONE_SHOT


# ---- pcp_upload_cloud_from_result -----------------------------------------------------------------------------------------

def _same_cloud(b, c, n_frames):
    assert b.n == c.n and b.lib.pcp_cloud_size(b.h) == c.lib.pcp_cloud_size(c.h) == c.n
    for f in range(n_frames):
        pb, pc = b.project_frame(f), c.project_frame(f)
        for k in ("cell", "pixel", "range", "xc", "yc", "zc"):
            assert np.array_equal(pb[k].view(np.uint32), pc[k].view(np.uint32)), (f, k)
    b.colorize(download=False)
    c.colorize(download=False)
    assert np.array_equal(_packed(b), _packed(c))


def test_upload_from_result_equals_upload_of_the_fetched_rows(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi

    o = _one_shot(gpu_ctx_factory)
    s, a, c = o["scene"], o["smooth_ctx"], o["colour_ctx"]
    m = len(o["rows"]["index"])
    b = gpu_ctx_factory()
    _views(b, capi, s, masks=True)
    b.set_label_fusion(True)
    assert b.upload_cloud_from_result(a) == m and m > 4 * CHUNK
    assert np.array_equal(a.mls_fetch(m)["xyz"], o["rows"]["xyz"]), "the source keeps its result"
    _same_cloud(b, c, 4)
    assert np.array_equal(b.colour_labels()["label"], c.colour_labels()["label"])
    # dst == src: the rows are copied aside, then the context holds them as its cloud
    d = gpu_ctx_factory()
    _views(d, capi, s, masks=True)
    d.set_label_fusion(True)
    d.upload_cloud(s["x"], s["y"], s["z"])
    assert d.cloud_smooth(_mls_params(capi)) == m
    assert d.upload_cloud_from_result(d) == m
    _same_cloud(d, c, 4)
    with pytest.raises(capi.PcpError) as e:  # the upload ended the result
        d.upload_cloud_from_result(d)
    assert e.value.code == capi.PCP_ERR_STATE


def test_upload_from_result_states_and_empty_result(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    s = small_scene
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    _views(b, capi, s)
    with pytest.raises(capi.PcpError) as e:  # nothing uploaded, nothing smoothed
        b.upload_cloud_from_result(a)
    assert e.value.code == capi.PCP_ERR_STATE
    a.upload_cloud(s["x"], s["y"], s["z"])
    with pytest.raises(capi.PcpError) as e:  # a cloud, but no smoothing result
        b.upload_cloud_from_result(a)
    assert e.value.code == capi.PCP_ERR_STATE and "no smoothing result" in str(e.value)
    # three points a metre apart: no point has the three neighbours a fit needs -> a result of 0 rows
    a.upload_cloud(np.array([0, 1, 2], np.float32), np.zeros(3, np.float32), np.ones(3, np.float32))
    p = capi.default_mls_params()
    p.upsampling = capi.UPSAMPLING_NONE
    assert a.mls_process(p) == 0
    b.upload_cloud(s["x"], s["y"], s["z"])
    assert b.upload_cloud_from_result(a) == 0 and b.lib.pcp_cloud_size(b.h) == 0
    col = b.colorize()
    assert col["rgb"].shape == (0, 3) and b.colour_compact()["count"] == 0


@pytest.mark.parametrize("rows", [1, 63, 65, 4097])
def test_upload_from_result_plane_padding_and_tile_edges(gpu_ctx_factory, small_scene, rows):
    """results of 1, 63, 65 and 4097 rows: MLS without upsampling on `rows` points in a 2 cm patch (every point has all the
    others within the 3 cm search radius, so every point is fitted).  A fit needs three neighbours, so no cloud of one point
    has a row: the result of 1 row is one query (pcp_mls_process_shard) of a cloud of four."""
    from pointcloudprocessor_amd import capi

    s = small_scene
    rng = np.random.default_rng(rows)
    n = max(rows, 4)  # a fit needs three neighbours
    x = (2.0 + rng.uniform(0, 0.02, n)).astype(np.float32)
    y = (-1.0 + rng.uniform(0, 0.02, n)).astype(np.float32)
    z = (1.5 + rng.normal(0, 1e-3, n)).astype(np.float32)
    a = gpu_ctx_factory()
    a.upload_cloud(x, y, z)
    p = capi.default_mls_params()
    p.upsampling = capi.UPSAMPLING_NONE
    if rows >= 4:
        assert a.mls_process(p) == rows
    else:
        assert a.mls_process_shard(p, 2, 3) == 1  # one query of the four points
    xyz = a.mls_fetch(rows)["xyz"]
    b, c = gpu_ctx_factory(), gpu_ctx_factory()
    for ctx in (b, c):
        _views(ctx, capi, s)
    assert b.upload_cloud_from_result(a) == rows
    c.upload_cloud_aos(xyz)
    _same_cloud(b, c, len(s["poses"]))
    assert np.array_equal(b.colour_compact()["xyz"].view(np.uint32), xyz[_packed(c) >> 24 != 0].view(np.uint32))


# ---- the depth-map accumulator ----------------------------------------------------------------------------------------------

def test_accumulator_merges_chunks_into_the_whole_clouds_maps(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    s = small_scene
    F = len(s["poses"])
    whole = gpu_ctx_factory()
    _views(whole, capi, s)
    whole.upload_cloud(s["x"], s["y"], s["z"])
    whole.depth_pass()
    ref = [whole.download_depth_map(f).view(np.uint32).copy() for f in range(F)]
    ctx = gpu_ctx_factory()
    _views(ctx, capi, s)
    bounds = [0, 1, 1 + 4097, len(s["x"])]
    ctx.depth_accum_reset()
    ptr, n = ctx.depth_accum_device()
    assert ptr and n == F * ref[0].size
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ctx.upload_cloud(s["x"][lo:hi], s["y"][lo:hi], s["z"][lo:hi])
        ctx.depth_pass()
        ctx.depth_accum_merge()
    lo, hi = bounds[-2], bounds[-1]
    ctx.upload_cloud(s["x"][lo:hi], s["y"][lo:hi], s["z"][lo:hi])
    ctx.depth_pass()
    own = [ctx.download_depth_map(f).view(np.uint32).copy() for f in range(F)]
    assert any(not np.array_equal(own[f], ref[f]) for f in range(F)), "the last chunk alone must not already be the whole"
    ctx.depth_accum_apply()
    for f in range(F):
        assert np.array_equal(ctx.download_depth_map(f).view(np.uint32), ref[f]), f
    # ... and the chunk coloured against the merged maps is the whole cloud's slice
    whole.colorize(download=False)
    ctx.colorize_from_depth(download=False)
    assert np.array_equal(_packed(ctx), _packed(whole)[lo:hi])


def test_accumulator_state_errors(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    s = small_scene
    ctx = gpu_ctx_factory()
    _views(ctx, capi, s)
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.depth_pass()

    def refused(call):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_STATE, e.value
        return str(e.value)

    for call in (ctx.depth_accum_merge, ctx.depth_accum_apply, ctx.depth_accum_device):  # before reset
        assert "pcp_depth_accum_reset" in refused(call)
    ctx.depth_accum_reset()
    ctx.depth_accum_merge()
    ctx.upload_cloud(s["x"][:100], s["y"][:100], s["z"][:100])  # the accumulator survives, the maps do not
    assert "pcp_depth_pass" in refused(ctx.depth_accum_merge)
    assert "pcp_depth_pass" in refused(ctx.depth_accum_apply)
    ctx.depth_pass(0, 2)  # not every keyframe
    refused(ctx.depth_accum_merge)
    ctx.depth_pass()
    ctx.depth_accum_merge()
    ctx.set_frames(s["poses"])  # drops it
    for call in (ctx.depth_accum_merge, ctx.depth_accum_apply, ctx.depth_accum_device):
        refused(call)
    cp = capi.default_cull_params()
    cp.cull_mode = capi.CULL_HPR
    ctx.set_camera(cam_struct(capi, s["cam"]), cp)
    for call in (ctx.depth_accum_reset, ctx.depth_accum_merge, ctx.depth_accum_apply, ctx.depth_accum_device):
        assert "PCP_CULL_HPR" in refused(call)


# ---- chunked equals one-shot -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fuse", [False, True])
def test_streamed_chain_equals_one_shot(gpu_ctx_factory, oracle, fuse):
    from pointcloudprocessor_amd import capi, pipeline

    o = _one_shot(gpu_ctx_factory)
    s, rows = o["scene"], o["rows"]
    has = o["has"] > 0
    assert has.mean() >= 0.9
    smooth, colour = pipeline.HipEngine(0), pipeline.HipEngine(0)
    try:
        smooth.ctx.upload_cloud(s["x"], s["y"], s["z"])
        _views(colour.ctx, capi, s, masks=fuse)
        cs = pipeline.CloudSmooth(smooth, _mls_params(capi))
        seen = []
        parts = list(cs.process_and_colourise_streamed(colour, CHUNK, fuse_labels=fuse, on_smoothed=seen.append))
        st = cs.streamed_colour
        print("streamed colour:", st)
        assert st["chunks"] >= 4 and len(parts) >= 4
        assert st["rows"] == len(rows["index"]) and st["coloured"] == int(has.sum())
        assert np.array_equal(np.concatenate([p["xyz"] for p in seen]).view(np.uint32), rows["xyz"].view(np.uint32))
        cat = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        assert np.array_equal(cat["index"], rows["index"][has])
        assert np.array_equal(cat["xyz"].view(np.uint32), rows["xyz"][has].view(np.uint32))
        assert np.array_equal(cat["rgb"], o["rgb"][has])
        assert ("label" in cat) == fuse
        if fuse:
            assert np.array_equal(cat["label"], o["label"][has])
            return
        # guard: the chunks coloured against their OWN maps only (no accumulator) are not the one-shot result
        ctx, col = smooth.ctx, colour.ctx
        ctx.upload_cloud(s["x"], s["y"], s["z"])
        _, _, chunks = ctx.cloud_smooth_stream_begin(_mls_params(capi), CHUNK)
        alone = []
        for _ in range(chunks):
            if ctx.cloud_smooth_stream_next() == 0:
                continue
            col.upload_cloud_from_result(ctx)
            col.depth_pass()
            col.colorize_from_depth(download=False)
            alone.append(_packed(col))
        ctx.cloud_smooth_stream_end()
        alone = np.concatenate(alone)
        one = o["rgb"][:, 0].astype(np.uint32) | o["rgb"][:, 1].astype(np.uint32) << 8 | o["rgb"][:, 2].astype(np.uint32) << 16 | \
            o["has"].astype(np.uint32) << 24
        differ = float((alone != one).mean())
        print("rows that differ when every chunk is coloured against its own maps:", differ)
        assert differ >= 0.10
    finally:
        smooth.close()
        colour.close()
    # independent anchor: the CPU oracle on the GPU's fetched rows
    ref = oracle.colorize(cam_struct(oracle, s["cam"]), oracle.default_cull_params(), rows["xyz"][:, 0].copy(), rows["xyz"][:, 1].copy(),
                          rows["xyz"][:, 2].copy(), s["poses"], s["images"], threads=8, want_top=False)
    assert np.array_equal(ref["has"] > 0, has)
    assert np.array_equal(ref["rgb"][has], cat["rgb"])


# ---- seek ----------------------------------------------------------------------------------------------------------------------

def test_stream_seek_re_emits_chunks(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi

    s = _levels_scene()
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    with pytest.raises(capi.PcpError) as e:
        ctx.cloud_smooth_stream_seek(0)
    assert e.value.code == capi.PCP_ERR_STATE
    _, kept, chunks = ctx.cloud_smooth_stream_begin(_mls_params(capi), CHUNK)
    assert chunks >= 4
    first = []
    for _ in range(chunks):
        m = ctx.cloud_smooth_stream_next()
        first.append(ctx.mls_fetch(m))
    assert sum(len(r["index"]) for r in first) == kept and all(len(r["index"]) for r in first)
    assert ctx.cloud_smooth_stream_next() == 0  # past the last chunk: the stream is still open
    for k in (chunks - 1, 0, 2, 2):
        ctx.cloud_smooth_stream_seek(k)
        again = ctx.mls_fetch(ctx.cloud_smooth_stream_next())
        for key in ("xyz", "normal", "curvature", "index"):
            assert np.array_equal(again[key].view(np.uint32), first[k][key].view(np.uint32)), (k, key)
    ctx.cloud_smooth_stream_seek(chunks)
    assert ctx.cloud_smooth_stream_next() == 0
    for bad in (-1, chunks + 1):
        with pytest.raises(capi.PcpError) as e:
            ctx.cloud_smooth_stream_seek(bad)
        assert e.value.code == capi.PCP_ERR_RANGE
    ctx.cloud_smooth_stream_end()
    with pytest.raises(capi.PcpError) as e:
        ctx.cloud_smooth_stream_seek(0)
    assert e.value.code == capi.PCP_ERR_STATE


# ---- pcp_colour_compact --------------------------------------------------------------------------------------------------------

def test_colour_compact_is_the_numpy_selection(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    s = small_scene
    ctx = gpu_ctx_factory()
    _views(ctx, capi, s, masks=True)
    xyz = np.stack([s["x"], s["y"], s["z"]], 1).astype(np.float32)
    with pytest.raises(capi.PcpError) as e:  # no colour result yet
        ctx.upload_cloud(s["x"], s["y"], s["z"])
        ctx.colour_compact()
    assert e.value.code == capi.PCP_ERR_STATE

    def check(col):
        sel = np.nonzero(col["has"])[0]
        assert 0 < len(sel) < len(xyz)
        got = ctx.colour_compact()
        assert got["count"] == len(sel)
        assert np.array_equal(got["index"], sel.astype(np.int32))
        assert np.array_equal(got["xyz"].view(np.uint32), xyz[sel].view(np.uint32))
        assert np.array_equal(got["rgb"], col["rgb"][sel])
        few = ctx.colour_compact(capacity=1000)  # the true count, the first rows
        assert few["count"] == len(sel) and len(few["index"]) == 1000
        assert np.array_equal(few["index"], sel[:1000]) and np.array_equal(few["rgb"], col["rgb"][sel[:1000]])
        return sel

    check(ctx.colorize())
    with pytest.raises(capi.PcpError) as e:  # a result made without fusion has no labels
        ctx.colour_compact(want_label=True)
    assert e.value.code == capi.PCP_ERR_STATE
    # after the local colour smoothing: the smoothed words, has = (r | g | b) != 0
    ctx.colour_smooth_local(0.05)
    w = _packed(ctx)
    sm = dict(rgb=np.stack([w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xff], 1).astype(np.uint8), has=(w >> 24).astype(np.uint8))
    check(sm)
    # with fusion: the fused label of the selected rows
    ctx.set_label_fusion(True)
    col = ctx.colorize()
    sel = check(col)
    assert np.array_equal(ctx.colour_compact(want_label=True)["label"], ctx.colour_labels()["label"][sel])
    ctx.set_label_fusion(False)
    # a cloud no keyframe sees
    ctx.upload_cloud(s["x"] + 500.0, s["y"], s["z"] - 500.0)
    assert not ctx.colorize()["has"].any()
    got = ctx.colour_compact()
    assert got["count"] == 0 and len(got["index"]) == 0
