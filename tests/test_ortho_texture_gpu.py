"""The orthophoto on the device ("Orthophotos") against the restatement in _ortho_texture_ref.py.  Every comparison
is exact equality of every layer and count.

The first scene is conftest's small_scene (20 000 points, 6 keyframes of 480 x 270): coloured, its coloured rows accumulated
into the map of _ortho_ref.down_frame(0.05) (242 x 202 pixels), filled at R = 2, textured at k = 4 (968 x 808 fine pixels).  By
the restatement with the interpolation off: 56 896 surface pixels, 45 853 textured, 21 039 with two views or more, 21 046 with
a view that lies in the image but fails the keep rule, 11 043 unseen; with the interpolation on (max_step 0.05): 45 863
textured, 21 059 with two or more, 11 033 unseen.  The second scene has the same cloud under make_trajectory(16) with 16
images: 60 487 textured, 9 485 pixels with five views or more, 5 439 with six or more (lists longer than M).  The preconditions
are asserted on the restatement's own counts."""
import numpy as np
import pytest

import _ortho_ref as oref
import _ortho_texture_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

_SCENES = {}
RECT = (202, 0, 40, 30)  # ortho pixels: the corner of the raster that holds most coloured rows, up to its right and top borders


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _scene(make, small_scene, frames, masks=True):
    """a context with the scene coloured and its map finished; the map's layers, the cloud's depth maps by the restatement and
    the restatements by parameters are computed once and shared"""
    key = (frames, masks)
    if key not in _SCENES:
        from pointcloudprocessor_amd import capi, synth

        s = dict(small_scene)
        if frames != len(s["poses"]):
            cd = s["cam"]
            s["poses"], s["ts"] = synth.make_trajectory(frames)
            s["images"] = [synth.make_image(f, cd["image_width"], cd["image_height"]) for f in range(frames)]
            s["masks"] = [synth.make_mask(f, cd["image_width"], cd["image_height"]) for f in range(frames)]
        ctx = make()
        ctx.set_camera(cam_struct(capi, s["cam"]))
        ctx.upload_cloud(s["x"], s["y"], s["z"])
        ctx.set_frames(s["poses"])
        for f, im in enumerate(s["images"]):
            ctx.upload_image(f, im)
            if masks:
                ctx.upload_mask(f, s["masks"][f])
        ctx.colorize(download=False)
        fr = oref.down_frame(0.05)
        ctx.ortho_begin(fr)
        ctx.ortho_add(0)
        ctx.ortho_finish(2)
        layers = _freeze(ctx.ortho_fetch())
        w2cs, dmaps = ref.depth_maps(s["cam"], s["poses"], s["x"], s["y"], s["z"])
        dmaps.setflags(write=False)
        _SCENES[key] = dict(ctx=ctx, s=s, fr=fr, map=layers, w2cs=w2cs, dmaps=dmaps, want={}, masks=s["masks"] if masks else None)
    return _SCENES[key]


def _want(b, k, views, interpolate, max_step=0.05, rect=None, gains=None):
    key = (k, views, interpolate, max_step, rect, None if gains is None else tuple(gains))
    if key not in b["want"]:
        s = b["s"]
        b["want"][key] = _freeze(ref.texture(s["cam"], s["poses"], s["images"], b["masks"], b["w2cs"], b["dmaps"], b["fr"], b["map"]["source"],
                                             b["map"]["depth"], k, views, interpolate, max_step, rect, gains))
    return b["want"][key]


def _same(got, want):
    bad = ref.same(got, want)
    if bad is not None and bad not in ref.COUNTS:
        n = int((got[bad] != want[bad]).reshape(got[bad].shape[0], got[bad].shape[1], -1).any(axis=2).sum())
        raise AssertionError(f"{bad} differs in {n} fine pixels")
    assert bad is None, f"{bad}: {got[bad]} != {want[bad]}"


@pytest.mark.parametrize("interpolate", [False, True])
@pytest.mark.parametrize("views", [1, 5])
def test_six_keyframes_equal_the_restatement(gpu_ctx_factory, small_scene, views, interpolate):
    b = _scene(gpu_ctx_factory, small_scene, 6)
    want = _want(b, 4, views, interpolate)
    print({k: v for k, v in want.items() if not isinstance(v, np.ndarray)})
    assert want["rgb"].shape == (808, 968, 3)
    # (with the interpolation on the restatement gives 45 863 / 21 059 / 21 037 / 11 033: the same floors hold)
    assert want["textured"] >= 40000 and want["two_or_more"] >= 15000 and want["refused_by_keep"] >= 15000 and want["unseen"] >= 5000
    assert (want["mask"] > 0).sum() >= 1000 and len(np.unique(want["view"])) == 7, "every keyframe is some pixel's best view"
    got = b["ctx"].ortho_texture(4, views, interpolate, 0.05)
    _same(got, want)
    assert got["skipped_pairs"] > 0, "the tile test skips pairs on this scene"
    if views == 5:  # the colour of a pixel with two views or more is a mean: it differs from the sharpest view's somewhere
        one = _want(b, 4, 1, interpolate)
        assert (one["rgb"] != want["rgb"]).any() and one["view"].tobytes() == want["view"].tobytes()


@pytest.mark.parametrize("views", [5, 3])
def test_sixteen_keyframes_lists_longer_than_the_views(gpu_ctx_factory, small_scene, views):
    b = _scene(gpu_ctx_factory, small_scene, 16)
    want = _want(b, 4, views, False)
    print({k: v for k, v in want.items() if not isinstance(v, np.ndarray)})
    assert want["five_or_more"] >= 5000 and want["six_or_more"] >= 2000
    assert want["count"].max() >= 8
    _same(b["ctx"].ortho_texture(4, views, False, 0.05), want)


@pytest.mark.parametrize("k", [1, 3, 16])
def test_scales_on_a_rectangle(gpu_ctx_factory, small_scene, k):
    b = _scene(gpu_ctx_factory, small_scene, 6)
    for interpolate in (False, True):
        want = _want(b, k, 5, interpolate, rect=RECT)
        assert want["rgb"].shape == (30 * k, 40 * k, 3) and want["textured"] >= 500 * k * k and want["unseen"] > 0 and (want["status"] == 0).any()
        _same(b["ctx"].ortho_texture(k, 5, interpolate, 0.05, rect=RECT), want)


def test_two_by_two_rectangles_make_the_whole_and_two_calls_agree(gpu_ctx_factory, small_scene):
    b = _scene(gpu_ctx_factory, small_scene, 6)
    ctx, fr = b["ctx"], b["fr"]
    want = _want(b, 4, 5, True)
    whole = ctx.ortho_texture(4, 5, True, 0.05)
    again = ctx.ortho_texture(4, 5, True, 0.05)
    for key in ref.LAYERS + ref.COUNTS + ("skipped_pairs",):
        a, c = whole[key], again[key]
        assert (a.tobytes() == c.tobytes()) if isinstance(a, np.ndarray) else a == c, key
    W, H, cx, cy = fr["width"], fr["height"], 181, 33  # (the coloured rows lie in columns 125..241, rows 0..68; 4 * 181 and 4 * 33 are no multiple of the tile)
    parts = [ctx.ortho_texture(4, 5, True, 0.05, rect=rect)
             for rect in ((0, 0, cx, cy), (cx, 0, W - cx, cy), (0, cy, cx, H - cy), (cx, cy, W - cx, H - cy))]
    joined = ref.tile(parts, 2, 2)
    for key in ref.LAYERS:
        assert joined[key].tobytes() == want[key].tobytes(), key
    for key in ref.COUNTS:
        assert sum(p[key] for p in parts) == want[key], key


def test_without_masks_the_mask_layer_is_zero(gpu_ctx_factory, small_scene):
    b = _scene(gpu_ctx_factory, small_scene, 6, masks=False)
    want = _want(b, 2, 5, True)
    assert not want["mask"].any() and want["textured"] >= 10000
    got = b["ctx"].ortho_texture(2, 5, True, 0.05)
    _same(got, want)
    assert not got["mask"].any()
    # the other layers are those of the scene with masks: a mask changes no colour
    with_masks = _want(_scene(gpu_ctx_factory, small_scene, 6), 2, 5, True)
    assert all(with_masks[key].tobytes() == want[key].tobytes() for key in ("rgb", "status", "view", "count")) and with_masks["mask"].any()


def test_gains(gpu_ctx_factory, small_scene):
    b = _scene(gpu_ctx_factory, small_scene, 6)
    ctx = b["ctx"]
    plain = _want(b, 4, 5, True)
    try:
        ctx.set_frame_gains(np.ones(6))
        _same(ctx.ortho_texture(4, 5, True, 0.05), plain)
        gains = np.random.default_rng(11).uniform(0.6, 1.4, 6)
        ctx.set_frame_gains(gains)
        for views in (5, 1):
            want = _want(b, 4, views, True, gains=[float(np.float32(g)) for g in gains])
            assert (want["rgb"] != _want(b, 4, views, True)["rgb"]).any(axis=2).sum() >= 30000 and (want["rgb"] == 255).sum() >= 100, \
                "the gains move the colours and some channels reach the clamp"
            _same(ctx.ortho_texture(4, views, True, 0.05), want)
    finally:
        ctx.set_frame_gains(None)
    _same(ctx.ortho_texture(4, 5, True, 0.05), plain)


def test_nothing_it_reads_changes(gpu_ctx_factory, small_scene):
    b = _scene(gpu_ctx_factory, small_scene, 6)
    ctx = b["ctx"]

    def state():
        m = ctx.ortho_fetch()
        return [m[key].tobytes() for key in oref.LAYERS] + [ctx.download_depth_map(f).tobytes() for f in range(6)] + \
               [ctx.download_result_packed().tobytes(), repr(ctx.ortho_stats())]

    before = state()
    assert before[:len(oref.LAYERS)] == [b["map"][key].tobytes() for key in oref.LAYERS]
    ctx.ortho_texture(4, 5, True, 0.05)
    ctx.ortho_texture(3, 1, False, 0.05, rect=RECT)
    assert state() == before
    # a later finish with another radius, and the texture of that map, behave as if the first texture had not run
    occupied, filled = ctx.ortho_finish(0)
    assert filled == 0
    bare = ctx.ortho_fetch()
    s = b["s"]
    want = ref.texture(s["cam"], s["poses"], s["images"], b["masks"], b["w2cs"], b["dmaps"], b["fr"], bare["source"], bare["depth"], 4, 5, True, 0.05)
    assert want["surface"] == 16 * occupied
    _same(ctx.ortho_texture(4, 5, True, 0.05), want)
    assert ctx.ortho_finish(2) == (int((b["map"]["status"] == 1).sum()), int((b["map"]["status"] == 2).sum()))
    assert state() == before
    _same(ctx.ortho_texture(4, 5, True, 0.05), _want(b, 4, 5, True))


def test_refusals_on_the_device(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    b = _scene(gpu_ctx_factory, small_scene, 6)
    ctx, fr = b["ctx"], b["fr"]
    W, H = fr["width"], fr["height"]
    for kw in (dict(scale=0), dict(scale=17), dict(scale=4, views=0), dict(scale=4, views=6), dict(scale=4, rect=(0, 0, 10, 0)),
               dict(scale=4, rect=(W - 9, 0, 10, 10)), dict(scale=4, rect=(0, H, 1, 1)), dict(scale=4, max_step=0.0),
               dict(scale=4, max_step=float("nan"))):
        with pytest.raises(capi.PcpError) as e:
            ctx.ortho_texture(**kw)
        assert e.value.code == capi.PCP_ERR_INVALID, kw
    _same(ctx.ortho_texture(4, 5, True, 0.05), _want(b, 4, 5, True))  # a refused call leaves everything as it was


def test_the_state_rules(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    s = small_scene
    ctx = gpu_ctx_factory()
    fr = oref.down_frame(0.05)

    def refused(what):
        with pytest.raises(capi.PcpError) as e:
            ctx.ortho_texture(2)
        assert e.value.code == capi.PCP_ERR_STATE, what
        assert what in str(e.value), str(e.value)

    refused("pcp_ortho_begin")  # no map
    ctx.ortho_begin(fr)
    refused("pcp_ortho_finish")  # not finished
    ctx.ortho_finish(0)
    refused("pcp_set_camera")
    ctx.set_camera(cam_struct(capi, s["cam"]))
    refused("pcp_set_frames")
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.set_frames(s["poses"])
    refused("no image uploaded for keyframe 0")
    for f in range(5):
        ctx.upload_image(f, s["images"][f])
    refused("no image uploaded for keyframe 5")
    ctx.upload_image(5, s["images"][5])
    refused("pcp_depth_pass has not covered keyframe 0")
    ctx.depth_pass(0, 3)
    refused("pcp_depth_pass has not covered keyframe 3")
    ctx.depth_pass()
    got = ctx.ortho_texture(2)  # an empty map: no surface anywhere
    assert got["surface"] == 0 and not got["status"].any() and (got["view"] == -1).all() and not got["rgb"].any()
    # a map of the cloud under hash colours, textured; then an upload invalidates the depth maps
    xyz = np.stack([s["x"], s["y"], s["z"]], axis=1)
    ctx.ortho_begin(fr)
    ctx.ortho_add_packed(np.full(len(xyz), 0x01808080, np.uint32))
    ctx.ortho_finish(1)
    m = ctx.ortho_fetch()
    w2cs, dmaps = ref.depth_maps(s["cam"], s["poses"], s["x"], s["y"], s["z"])
    want = ref.texture(s["cam"], s["poses"], s["images"], None, w2cs, dmaps, fr, m["source"], m["depth"], 2, 1, True, 0.05)
    assert want["surface"] >= 100000 and want["textured"] >= 5000
    _same(ctx.ortho_texture(2), want)
    ctx.upload_cloud(s["x"][:1000], s["y"][:1000], s["z"][:1000])
    refused("pcp_depth_pass has not covered keyframe 0")
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.depth_pass()
    _same(ctx.ortho_texture(2), want)
    # the culls without depth maps are refused, as pcp_depth_accum_* refuses them
    for change in (dict(cull_mode=capi.CULL_HPR_CANDIDATES), dict(cull_mode=capi.CULL_HPR), dict(enable_depth_buffer_culling=0)):
        cull = capi.default_cull_params()
        for key, v in change.items():
            setattr(cull, key, v)
        ctx.set_camera(cam_struct(capi, s["cam"]), cull)
        refused("PCP_CULL_ZBUFFER")
    # the view layer is int16: 32 766 keyframes are the most it names (refused with the keyframes, before their images are asked for)
    ctx.set_frames(np.tile(np.asarray(s["poses"], np.float64).reshape(-1, 7)[:1], (32767, 1)))
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_texture(2)
    assert e.value.code == capi.PCP_ERR_RANGE and "32766" in str(e.value)
    ctx.set_frames(s["poses"])
    ctx.ortho_end()
    refused("pcp_ortho_begin")
