"""Orthophotos of unrolled maps on the device ("Orthophotos of unrolled maps") against the restatement in
_ortho_cyl_texture_ref.py.  Every comparison is exact equality of every layer and count.

The scene is _ortho_cyl_texture_ref's: a vault of R 3 (an open arc, 291 x 77 map pixels of 2 cm, seen from inside, side +1) and,
between it and the six keyframes of 480 x 270, a closed pier of R 0.3 (189 x 70 pixels of 1 cm, seen from outside, side -1, its
seam on the seen side).  Each structure's map holds every point of the cloud inside its depth window (ortho_add_packed with every
has bit set), so it does not depend on the colours.  By the restatement at k = 4, views 5, interpolation on: the vault has
353 568 surface pixels, 159 006 textured, 132 767 with two views or more, 55 519 with a view inside an image that the depth map
hides (the pier stands in front), 194 562 unseen; the pier 206 672 / 97 329 / 80 105 / 150 043 / 109 343 (its far side).  The
coverage conditions are asserted on the restatement's own counts."""
import numpy as np
import pytest

import _ortho_cyl_texture_ref as ref
import _ortho_ref as oref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

MAX_STEP = 0.004  # metres: cuts the interpolation across some neighbours of either map and not across most
_SCENES = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _scene(make, name, masks=True):
    """a context with the cloud coloured and the structure's unrolled map finished; the map's layers, the cloud's depth maps by
    the restatement and the restatements by parameters are computed once and shared"""
    key = (name, masks)
    if key not in _SCENES:
        from pointcloudprocessor_amd import capi, synth

        if "inputs" not in _SCENES:
            cam = synth.camera_dict("tiny")
            pts, poses = ref.scene_points(), ref.scene_poses()
            w, h = cam["image_width"], cam["image_height"]
            w2cs, dmaps = ref.depth_maps(cam, poses, pts[:, 0], pts[:, 1], pts[:, 2])
            dmaps.setflags(write=False)
            pts.setflags(write=False)
            _SCENES["inputs"] = dict(cam=cam, pts=pts, poses=poses, w2cs=w2cs, dmaps=dmaps, images=[synth.make_image(f, w, h) for f in range(6)],
                                     masks=[synth.make_mask(f, w, h) for f in range(6)])
        s = _SCENES["inputs"]
        fr = ref.scene_frames()[name]
        ctx = make()
        ctx.set_camera(cam_struct(capi, s["cam"]))
        ctx.upload_cloud(s["pts"][:, 0].copy(), s["pts"][:, 1].copy(), s["pts"][:, 2].copy())
        ctx.set_frames(s["poses"])
        for f, im in enumerate(s["images"]):
            ctx.upload_image(f, im)
            if masks:
                ctx.upload_mask(f, s["masks"][f])
        ctx.colorize(download=False)
        ctx.ortho_begin_cyl(fr)
        ctx.ortho_add_packed(np.full(len(s["pts"]), 0x01808080, np.uint32))
        ctx.ortho_finish(ref.SCENE_FILL[name])
        _SCENES[key] = dict(ctx=ctx, s=s, fr=fr, map=_freeze(ctx.ortho_fetch()), want={}, masks=s["masks"] if masks else None)
    return _SCENES[key]


def _want(b, k, views, interpolate, max_step=MAX_STEP, rect=None, gains=None):
    key = (k, views, interpolate, max_step, rect, None if gains is None else tuple(gains))
    if key not in b["want"]:
        s = b["s"]
        b["want"][key] = _freeze(ref.texture(s["cam"], s["poses"], s["images"], b["masks"], s["w2cs"], s["dmaps"], b["fr"], b["map"]["source"],
                                             b["map"]["depth"], k, views=views, interpolate=interpolate, max_step=max_step, rect=rect, gains=gains))
    return b["want"][key]


def _same(got, want):
    bad = ref.same(got, want)
    if bad is not None and bad not in ref.COUNTS:
        n = int((got[bad] != want[bad]).reshape(got[bad].shape[0], got[bad].shape[1], -1).any(axis=2).sum())
        raise AssertionError(f"{bad} differs in {n} fine pixels")
    assert bad is None, f"{bad}: {got[bad]} != {want[bad]}"


@pytest.mark.parametrize("name", ["vault", "pier"])
def test_the_map_is_the_host_twins_and_the_restatement_covers_the_cases(gpu_ctx_factory, name):
    """the coverage conditions, on the restatement alone (CPU): at k = 4, of the surface pixels, at least 30 % textured, 1 000 with
    two views or more, 1 000 with a view inside an image that the depth map hides, 100 with status 2"""
    from pointcloudprocessor_amd import capi

    b = _scene(gpu_ctx_factory, name)
    fr, s = b["fr"], b["s"]
    host = capi.ortho_cyl_host(fr, s["pts"], np.full((len(s["pts"]), 3), 0x80, np.uint8), fill_radius=ref.SCENE_FILL[name])
    assert all(host[key].tobytes() == b["map"][key].tobytes() for key in ("index", "depth", "rgb", "status", "source"))
    assert 160 * 30 <= fr["width"] * fr["height"] <= 320 * 80
    assert (4 * fr["width"]) % 16 and (4 * fr["height"]) % 16, "the fine raster's sides are no multiples of the tile"
    want = _want(b, 4, 5, True)
    print(name, {k: v for k, v in want.items() if not isinstance(v, np.ndarray)}, "status 2:", int((want["status"] == 2).sum()),
          "mask pixels", int((want["mask"] > 0).sum()), "best views", np.unique(want["view"]).tolist())
    assert want["textured"] >= 0.30 * want["surface"]
    assert want["two_or_more"] >= 1000
    assert want["refused_by_keep"] >= 1000
    assert (want["status"] == 2).sum() >= 100 and (want["status"] == 0).sum() >= 100
    assert (want["mask"] > 0).sum() >= 1000 and want["count"].max() >= 5


@pytest.mark.parametrize("interpolate", [False, True])
@pytest.mark.parametrize("views", [1, 5])
@pytest.mark.parametrize("name", ["vault", "pier"])
def test_the_whole_raster_equals_the_restatement(gpu_ctx_factory, name, views, interpolate):
    b = _scene(gpu_ctx_factory, name)
    want = _want(b, 4, views, interpolate)
    assert want["rgb"].shape == (4 * b["fr"]["height"], 4 * b["fr"]["width"], 3)
    got = b["ctx"].ortho_texture_cyl(4, views, interpolate, MAX_STEP)
    _same(got, want)
    assert got["skipped_pairs"] > 0, "the tile test skips pairs on this scene"
    if views == 5:  # the colour of a pixel with two views or more is a mean: it differs from the sharpest view's somewhere
        one = _want(b, 4, 1, interpolate)
        assert (one["rgb"] != want["rgb"]).any() and one["view"].tobytes() == want["view"].tobytes()
    if interpolate:
        assert (want["rgb"] != _want(b, 4, views, False)["rgb"]).any(), "the interpolated depth moves some texels"


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("name", ["vault", "pier"])
def test_scales_on_a_rectangle(gpu_ctx_factory, name, k):
    """on the ring a rectangle up to the raster's last column, where theta is largest (2 pi, and past it within that column: the
    seam faces the keyframes); on the vault one about the middle of the arc, which the keyframes see"""
    b = _scene(gpu_ctx_factory, name)
    W = b["fr"]["width"]
    rect = (W - 37, 11, 37, 23) if name == "pier" else (127, 11, 37, 23)
    for interpolate in (False, True):
        want = _want(b, k, 5, interpolate, rect=rect)
        assert want["rgb"].shape == (23 * k, 37 * k, 3) and want["surface"] >= 500 * k * k and want["textured"] >= 300 * k * k
        if name == "pier":
            assert (want["status"][:, -k:] == 1).any(), "the last column is textured"
        _same(b["ctx"].ortho_texture_cyl(k, 5, interpolate, MAX_STEP, rect=rect), want)


@pytest.mark.parametrize("name", ["vault", "pier"])
def test_two_by_two_rectangles_make_the_whole_and_two_calls_agree(gpu_ctx_factory, name):
    b = _scene(gpu_ctx_factory, name)
    ctx, fr = b["ctx"], b["fr"]
    want = _want(b, 4, 5, True)
    whole = ctx.ortho_texture_cyl(4, 5, True, MAX_STEP)
    again = ctx.ortho_texture_cyl(4, 5, True, MAX_STEP)
    for key in ref.LAYERS + ref.COUNTS + ("skipped_pairs",):
        a, c = whole[key], again[key]
        assert (a.tobytes() == c.tobytes()) if isinstance(a, np.ndarray) else a == c, key
    W, H, cx, cy = fr["width"], fr["height"], 131, 29  # (4 * 131 and 4 * 29 are no multiple of the tile)
    parts = [ctx.ortho_texture_cyl(4, 5, True, MAX_STEP, rect=rect)
             for rect in ((0, 0, cx, cy), (cx, 0, W - cx, cy), (0, cy, cx, H - cy), (cx, cy, W - cx, H - cy))]
    joined = ref.tile(parts, 2, 2)
    for key in ref.LAYERS:
        assert joined[key].tobytes() == want[key].tobytes(), key
    for key in ref.COUNTS:
        assert sum(p[key] for p in parts) == want[key], key


def test_without_masks_the_mask_layer_is_zero(gpu_ctx_factory):
    b = _scene(gpu_ctx_factory, "pier", masks=False)
    want = _want(b, 3, 5, True)
    assert not want["mask"].any() and want["textured"] >= 10000
    got = b["ctx"].ortho_texture_cyl(3, 5, True, MAX_STEP)
    _same(got, want)
    with_masks = _want(_scene(gpu_ctx_factory, "pier"), 3, 5, True)
    assert all(with_masks[key].tobytes() == want[key].tobytes() for key in ("rgb", "status", "view", "count")) and with_masks["mask"].any()


def test_gains(gpu_ctx_factory):
    b = _scene(gpu_ctx_factory, "vault")
    ctx = b["ctx"]
    plain = _want(b, 4, 5, True)
    try:
        ctx.set_frame_gains(np.ones(6))
        _same(ctx.ortho_texture_cyl(4, 5, True, MAX_STEP), plain)
        gains = np.random.default_rng(11).uniform(0.6, 1.4, 6)
        ctx.set_frame_gains(gains)
        for views in (5, 1):
            want = _want(b, 4, views, True, gains=[float(np.float32(g)) for g in gains])
            assert (want["rgb"] != _want(b, 4, views, True)["rgb"]).any(axis=2).sum() >= 30000 and (want["rgb"] == 255).sum() >= 100, \
                "the gains move the colours and some channels reach the clamp"
            _same(ctx.ortho_texture_cyl(4, views, True, MAX_STEP), want)
    finally:
        ctx.set_frame_gains(None)
    _same(ctx.ortho_texture_cyl(4, 5, True, MAX_STEP), plain)


@pytest.mark.parametrize("name", ["vault", "pier"])
def test_nothing_it_reads_changes(gpu_ctx_factory, name):
    b = _scene(gpu_ctx_factory, name)
    ctx = b["ctx"]

    def state():
        m = ctx.ortho_fetch()
        return [m[key].tobytes() for key in ("index", "depth", "rgb", "status", "source")] + \
               [ctx.download_depth_map(f).tobytes() for f in range(6)] + [ctx.download_result_packed().tobytes(), repr(ctx.ortho_stats())]

    before = state()
    assert before[:5] == [b["map"][key].tobytes() for key in ("index", "depth", "rgb", "status", "source")]
    first = ctx.ortho_texture_cyl(4, 5, True, MAX_STEP)
    ctx.ortho_texture_cyl(3, 1, False, MAX_STEP, rect=(5, 5, 40, 30))
    second = ctx.ortho_texture_cyl(4, 5, True, MAX_STEP)
    assert state() == before
    assert all(first[key].tobytes() == second[key].tobytes() for key in ref.LAYERS)


def test_the_state_rules_by_code_and_message(gpu_ctx_factory):
    """each call refuses the other kind of map by name, and the new one keeps OT1's checks in OT1's order"""
    from pointcloudprocessor_amd import capi

    s = _scene(gpu_ctx_factory, "pier")["s"]
    fr = ref.scene_frames()["pier"]
    ctx = gpu_ctx_factory()

    def refused(what, call=None):
        with pytest.raises(capi.PcpError) as e:
            (call or ctx.ortho_texture_cyl)(2)
        assert e.value.code == capi.PCP_ERR_STATE, (what, e.value.code)
        assert what in str(e.value), str(e.value)
        return str(e.value)

    refused("pcp_ortho_begin")  # no map
    ctx.ortho_begin(oref.down_frame(0.05))
    msg = refused("pcp_ortho_texture", ctx.ortho_texture_cyl)  # a live planar map: the second check, before "not finished"
    assert "pcp_ortho_texture_cyl: the live map is a plane's" in msg
    refused("pcp_ortho_finish", ctx.ortho_texture)
    ctx.ortho_begin_cyl(fr)
    msg = refused("orthophotos of unrolled maps are not built", ctx.ortho_texture)
    assert "pcp_ortho_texture_cyl" in msg
    refused("pcp_ortho_finish")  # not finished
    ctx.ortho_finish(0)
    refused("pcp_set_camera")
    ctx.set_camera(cam_struct(capi, s["cam"]))
    refused("pcp_set_frames")
    ctx.upload_cloud(s["pts"][:, 0].copy(), s["pts"][:, 1].copy(), s["pts"][:, 2].copy())
    ctx.set_frames(s["poses"])
    refused("no image uploaded for keyframe 0")
    for f in range(6):
        ctx.upload_image(f, s["images"][f])
    refused("pcp_depth_pass has not covered keyframe 0")
    ctx.depth_pass()
    got = ctx.ortho_texture_cyl(2)  # an empty map: no surface anywhere
    assert got["surface"] == 0 and not got["status"].any() and (got["view"] == -1).all() and not got["rgb"].any()
    W, H = fr["width"], fr["height"]
    for kw in (dict(scale=0), dict(scale=17), dict(scale=4, views=0), dict(scale=4, views=6), dict(scale=4, rect=(0, 0, 10, 0)),
               dict(scale=4, rect=(W - 9, 0, 10, 10)), dict(scale=4, rect=(0, H, 1, 1)), dict(scale=4, max_step=0.0),
               dict(scale=4, max_step=float("nan"))):
        with pytest.raises(capi.PcpError) as e:
            ctx.ortho_texture_cyl(**kw)
        assert e.value.code == capi.PCP_ERR_INVALID and "pcp_ortho_texture_cyl" in str(e.value), kw
    cull = capi.default_cull_params()
    cull.cull_mode = capi.CULL_HPR
    ctx.set_camera(cam_struct(capi, s["cam"]), cull)
    refused("PCP_CULL_ZBUFFER")
    ctx.ortho_end()
    refused("pcp_ortho_begin")
    refused("pcp_ortho_begin", ctx.ortho_texture)
