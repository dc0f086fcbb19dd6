"""The mask distance maps on the device ("Mask distance maps"): pcp_mask_edt / pcp_mask_edt_frames against the
library's CPU form and against the brute-force restatement in _mask_edt_ref.py, both outputs bit for bit, and the distance
against scipy.ndimage.distance_transform_edt.  The restatement compares every background pixel with every pixel, so it
covers a whole image while pixels x background pixels <= 2e8 and 512 pixels drawn with a fixed seed beyond that (the three
270 x 480 scenes and the densest masks of the widest image); the CPU form and scipy always cover the whole image."""
import numpy as np
import pytest
import scipy.ndimage

import _mask_edt_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

TWIN_BUDGET = 2e8
# beside the CPU suite's shapes: a row wider than one workgroup and than 4096, a tall column (40 segments of 64 rows), and the
# widest row the limit allows (64 KB of LDS)
EXTRA_SHAPES = [(3, 4100), (2500, 2), (2, 16384)]
SCENE = (270, 480)


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


_CTX = {}


def _ctx(make, small_scene):
    """one context for the module: six keyframes and the few points pcp_upload_mask asks for; every test sets its own camera"""
    if not _CTX:
        ctx = make()
        _CTX["ctx"] = ctx
        _resize(ctx, small_scene, SCENE)
        ctx.upload_cloud(small_scene["x"][:64], small_scene["y"][:64], small_scene["z"][:64])
        ctx.set_frames(small_scene["poses"])
    return _CTX["ctx"]


def _resize(ctx, small_scene, shape):
    capi = _capi()
    cam = dict(small_scene["cam"])
    cam["image_height"], cam["image_width"] = shape
    ctx.set_camera(cam_struct(capi, cam), capi.default_cull_params())  # (drops every uploaded image and mask)


def _compare(got_d2, got_nearest, mask, threshold=0, scipy_too=False):
    host = _capi().mask_edt_host(mask, threshold)
    assert got_d2.dtype == np.uint32 and got_nearest.dtype == np.int32 and got_d2.shape == mask.shape
    assert np.array_equal(got_d2, host["d2"])
    assert np.array_equal(got_nearest, host["nearest"])
    background = int((mask <= threshold).sum())
    if background == 0:
        assert (got_d2 == ref.SENTINEL_D2).all() and (got_nearest == -1).all()
        return
    if background * mask.size <= TWIN_BUDGET:
        want_d2, want_nearest = ref.edt(mask, threshold)
        assert np.array_equal(got_d2, want_d2) and np.array_equal(got_nearest, want_nearest)
    else:
        pixels = np.random.default_rng(99).choice(mask.size, 512, replace=False)
        want_d2, want_nearest = ref.edt_at(mask, pixels, threshold)
        assert np.array_equal(got_d2.ravel()[pixels], want_d2) and np.array_equal(got_nearest.ravel()[pixels], want_nearest)
    if scipy_too:
        assert np.array_equal(np.sqrt(got_d2.astype(np.float64)), scipy.ndimage.distance_transform_edt(mask > threshold))


@pytest.mark.parametrize("shape", ref.SHAPES + EXTRA_SHAPES, ids=lambda s: "%dx%d" % s)
def test_device_equals_host_form_and_restatement(gpu_ctx_factory, small_scene, shape):
    ctx = _ctx(gpu_ctx_factory, small_scene)
    _resize(ctx, small_scene, shape)
    masks = [ref.random_mask(shape, d, seed=1000 * shape[0] + shape[1]) for d in ref.DENSITIES]
    masks.append(ref.corner_mask(shape))
    for f, m in enumerate(masks):
        ctx.upload_mask(f, m)
    out = ctx.mask_edt_frames(0, len(masks))
    assert out["d2"].shape == (len(masks),) + shape
    for f, m in enumerate(masks):
        _compare(out["d2"][f], out["nearest"][f], m, scipy_too=shape[0] * shape[1] <= 70 * 70)
    one = ctx.mask_edt(2)
    assert np.array_equal(one["d2"], out["d2"][2]) and np.array_equal(one["nearest"], out["nearest"][2])


@pytest.fixture(scope="module")
def scene_masks(small_scene):
    """the 270 x 480 masks: small_scene's six disc masks (blobs, long searches), one background pixel in the far corner (the
    worst case of the outward search) and thin random-walk cracks; read-only"""
    masks = dict(discs=list(small_scene["masks"]), corner=[ref.corner_mask(SCENE)], cracks=[ref.crack_mask(SCENE, seed=k) for k in (1, 2)])
    for group in masks.values():
        for m in group:
            assert m.shape == SCENE
    return masks


@pytest.mark.parametrize("kind", ["discs", "corner", "cracks"])
def test_scenes_against_host_form_restatement_and_scipy(gpu_ctx_factory, small_scene, scene_masks, kind):
    ctx = _ctx(gpu_ctx_factory, small_scene)
    _resize(ctx, small_scene, SCENE)
    masks = scene_masks[kind]
    for f, m in enumerate(masks):
        ctx.upload_mask(f, m)
    out = ctx.mask_edt_frames(0, len(masks))
    for f, m in enumerate(masks):
        assert 0 < int((m > 0).sum()) < m.size
        _compare(out["d2"][f], out["nearest"][f], m, scipy_too=True)
    if kind == "corner":
        assert out["d2"][0][0, 0] == 269 ** 2 + 479 ** 2 and (out["nearest"][0] == 270 * 480 - 1).all()
    if kind == "discs":  # the batched call is the six single calls, with and without the second output
        for f in range(len(masks)):
            one = ctx.mask_edt(f)
            assert np.array_equal(one["d2"], out["d2"][f]) and np.array_equal(one["nearest"], out["nearest"][f])
        part = ctx.mask_edt_frames(2, 3, want_nearest=False)
        assert set(part) == {"d2"} and np.array_equal(part["d2"], out["d2"][2:5])


def test_thresholds_and_the_tie_case(gpu_ctx_factory, small_scene):
    ctx = _ctx(gpu_ctx_factory, small_scene)
    shape = (45, 70)
    _resize(ctx, small_scene, shape)
    mask = ref.byte_mask(shape, seed=7)
    ctx.upload_mask(0, mask)
    for t in (0, 127, 254, 255):
        out = ctx.mask_edt(0, t)
        _compare(out["d2"], out["nearest"], mask, t, scipy_too=True)
    _resize(ctx, small_scene, (5, 5))
    ctx.upload_mask(1, ref.tie_mask())
    out = ctx.mask_edt(1)
    _compare(out["d2"], out["nearest"], ref.tie_mask())
    assert out["d2"][2, 2] == 4 and out["nearest"][2, 2] == 2


def test_a_later_image_upload_and_the_texels(gpu_ctx_factory, small_scene):
    """the colour shares the texel with the mask: uploading the colour afterwards changes nothing, and the call leaves the
    texels as they were"""
    ctx = _ctx(gpu_ctx_factory, small_scene)
    _resize(ctx, small_scene, SCENE)
    mask = small_scene["masks"][3]
    ctx.upload_image(1, small_scene["images"][1])
    ctx.upload_mask(1, mask)
    bgr0, mask0 = ctx.download_image(1)
    assert np.array_equal(mask0, mask)
    first = ctx.mask_edt(1)
    bgr1, mask1 = ctx.download_image(1)
    assert bgr0.tobytes() == bgr1.tobytes() and mask0.tobytes() == mask1.tobytes()
    ctx.upload_image(1, small_scene["images"][4])
    again = ctx.mask_edt(1)
    assert np.array_equal(first["d2"], again["d2"]) and np.array_equal(first["nearest"], again["nearest"])
    bgr2, mask2 = ctx.download_image(1)
    assert mask2.tobytes() == mask0.tobytes() and bgr2.tobytes() != bgr0.tobytes()


def test_error_returns(gpu_ctx_factory, small_scene):
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory, small_scene)
    _resize(ctx, small_scene, (9, 11))  # (no keyframe has a mask now)
    ctx.upload_mask(0, np.zeros((9, 11), np.uint8))
    ctx.upload_image(1, np.zeros((9, 11, 3), np.uint8))

    def code(fn, *a):
        with pytest.raises(capi.PcpError) as e:
            fn(*a)
        return e.value.code, str(e.value)

    assert ctx.mask_edt(0)["d2"].shape == (9, 11)
    assert code(ctx.mask_edt, 1)[0] == capi.PCP_ERR_STATE  # an image, but no mask
    rc, msg = code(ctx.mask_edt, 2)
    assert rc == capi.PCP_ERR_STATE and "pcp_upload_mask" in msg and "keyframe 2" in msg
    assert code(ctx.mask_edt_frames, 0, 2)[0] == capi.PCP_ERR_STATE
    assert code(ctx.mask_edt, 6)[0] == capi.PCP_ERR_RANGE
    assert code(ctx.mask_edt, -1)[0] == capi.PCP_ERR_RANGE
    assert code(ctx.mask_edt_frames, 5, 2)[0] == capi.PCP_ERR_RANGE
    assert code(ctx.mask_edt_frames, 0, -1)[0] == capi.PCP_ERR_RANGE
    assert code(ctx.mask_edt, 0, 256)[0] == capi.PCP_ERR_INVALID
    assert code(ctx.mask_edt, 0, -1)[0] == capi.PCP_ERR_INVALID
    assert ctx.mask_edt_frames(0, 0)["d2"].shape == (0, 9, 11)
    _resize(ctx, small_scene, (1, 16385))
    ctx.upload_mask(0, np.zeros((1, 16385), np.uint8))
    rc, msg = code(ctx.mask_edt, 0)
    assert rc == capi.PCP_ERR_RANGE and "16384" in msg


def test_a_colour_run_is_untouched_by_calls_in_between(gpu_ctx_factory, small_scene):
    capi = _capi()
    s = small_scene
    ctx = gpu_ctx_factory()
    ctx.set_camera(cam_struct(capi, s["cam"]), capi.default_cull_params())
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.set_frames(s["poses"])
    for f, (im, mk) in enumerate(zip(s["images"], s["masks"])):
        ctx.upload_image(f, im)
        ctx.upload_mask(f, mk)
    before = ctx.colorize()
    packed = ctx.download_result_packed().copy()
    maps = ctx.mask_edt_frames(0, len(s["masks"]))
    assert np.array_equal(ctx.download_result_packed(), packed)  # the colour result in place
    ctx.mask_edt(3, 100)
    after = ctx.colorize()
    assert before["rgb"].tobytes() == after["rgb"].tobytes() and before["has"].tobytes() == after["has"].tobytes()
    host = capi.mask_edt_host(s["masks"][5])
    assert np.array_equal(maps["d2"][5], host["d2"]) and np.array_equal(maps["nearest"][5], host["nearest"])
