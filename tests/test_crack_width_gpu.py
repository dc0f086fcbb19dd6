"""The crack width maps on the device ("Crack width maps"): pcp_crack_width against the library's CPU form and the
restatement in _crack_width_ref.py, both fed the position image pcp_frame_geometry returns for the same keyframe -- flags
bits 0-3, edges, w2d2 and all 13 moments by exact equality (the restatement's moments at 600 seeded sites where an image has
more; its traces need the distance maps, which come from pcp_mask_edt_host, pinned by its own suite) -- and the float stage
against the fp64 twin on a 270 x 480 crack scene.

Float stage, measured on an MI355X (test_float_stage_against_the_fp64_twin prints them): 17 288 compared sites, normal 3.0e-8
(gate 1e-4), relative width error 5.9e-8 (bound 6.9e-4 at cos_min 0.506), points 5.5e-8 relative."""
import numpy as np
import pytest

import _crack_width_ref as ref
import _mask_edt_ref as edt_ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

EXTRA_SHAPES = [(3, 4100), (2500, 2)]  # a row wider than four rounds of the row scan; 40 segments of the column scan
SCENE = (270, 480)
FRAMES = 6
ALL = ("flags", "edges", "w2d2", "width", "points", "plane", "moments")


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


_STATE = {}


def _ctx(make):
    if "ctx" not in _STATE:
        _STATE["ctx"] = make()
    return _STATE["ctx"]


def _cull(capi):
    cull = capi.default_cull_params()
    cull.enable_depth_buffer_culling = 0  # every projecting point contributes: the points beyond 64 m reach the position image
    return cull


def _setup(ctx, shape, cloud=None, seed=None):
    """camera of `shape`, the wall cloud (or `cloud`), FRAMES identity keyframes; returns the position image of keyframe 0"""
    capi = _capi()
    ctx.set_camera(cam_struct(capi, ref.camera(shape)), _cull(capi))  # (drops every uploaded image and mask)
    if cloud is None:
        _, c2w = capi.pose_to_matrices(ref.IDENTITY_POSE)
        cloud = ref.wall_cloud(shape, seed=shape[0] * 31 + shape[1] if seed is None else seed, c2w=c2w)
    ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
    ctx.set_frames(np.tile(ref.IDENTITY_POSE, (FRAMES, 1)))
    geo = ctx.frame_geometry(0, normals=False)
    return geo, cloud


def _compare(ctx, frame, mask, geo, threshold, radius):
    capi = _capi()
    got = ctx.crack_width(frame, threshold, radius, want=ALL)
    host = capi.crack_width_host(mask, geo["index"], geo["xyz_cam"], threshold, radius)
    assert got["flags"].dtype == np.uint8 and got["flags"].shape == mask.shape and got["edges"].shape == mask.shape + (4,)
    assert np.array_equal(got["flags"] & ref.INTEGER_BITS, host["flags"])
    assert np.array_equal(got["edges"], host["edges"]) and np.array_equal(got["w2d2"], host["w2d2"])
    assert np.array_equal(got["moments"], host["moments"])
    maps = capi.mask_edt_host(mask, threshold)
    ref.check_integers(got, mask, geo["index"], geo["xyz_cam"], threshold, radius, d2=maps["d2"], nearest=maps["nearest"])
    f = got["flags"]
    site, width, plane = (f & ref.SITE) != 0, (f & ref.WIDTH) != 0, (f & ref.PLANE) != 0
    need = ref.NEAR | ref.FAR | ref.PLANE | ref.RAYS
    assert np.array_equal(width, (f & need) == need) and not (f & 0x80).any() and not f[~site].any()
    assert got["sites"] == int(site.sum()) and got["widths"] == int(width.sum())
    assert not got["width"][~width].any() and not got["points"][~width].any() and not got["plane"][~plane].any()
    assert (got["width"][width] > 0).all() and np.isfinite(got["points"]).all()
    can = site & (got["moments"][..., 0] >= 3) & (maps["d2"] != 0xFFFFFFFF)
    assert not (plane & ~can).any()
    if mask.shape == SCENE:
        assert np.array_equal(plane, can)  # (the wall's windows span a plane: every such normal is finite)
    return got


@pytest.mark.parametrize("shape", edt_ref.SHAPES + EXTRA_SHAPES, ids=lambda s: "%dx%d" % s)
def test_device_equals_host_form_and_restatement(gpu_ctx_factory, shape):
    ctx = _ctx(gpu_ctx_factory)
    geo, _ = _setup(ctx, shape)
    masks = ref.masks(shape, seed=shape[0] + 7 * shape[1])
    cases = [("half", 0, 1), ("cracks", 0, 3), ("corner", 0, 7), ("dense", 0, 150), ("full", 0, 150), ("bytes", 127, 3)]
    for f, (name, _, _) in enumerate(cases):
        ctx.upload_mask(f, masks[name])
    widths = 0
    for f, (name, t, radius) in enumerate(cases):
        got = _compare(ctx, f, masks[name], geo, t, radius)
        widths += got["widths"]
        if name == "full":
            assert (got["flags"] == ref.SITE).all() and (got["edges"] == -1).all() and not got["width"].any()
    if shape[0] >= 33 and shape[1] >= 64:
        assert widths > 0
    again = ctx.crack_width(2, 0, 7, want=("edges",))  # fewer outputs: the same bytes
    assert set(again) == {"edges", "sites", "widths"}
    assert np.array_equal(again["edges"], capi_edges(masks["corner"], geo, 7))


def capi_edges(mask, geo, radius):
    return _capi().crack_width_host(mask, geo["index"], geo["xyz_cam"], 0, radius)["edges"]


@pytest.fixture(scope="module")
def scene_masks(small_scene):
    masks = dict(discs=small_scene["masks"][0], corner=edt_ref.corner_mask(SCENE), cracks=edt_ref.crack_mask(SCENE, seed=4, cracks=12))
    for m in masks.values():
        assert m.shape == SCENE
    return masks


@pytest.mark.parametrize("kind", ["discs", "corner", "cracks"])
def test_scenes_at_radius_150(gpu_ctx_factory, scene_masks, kind):
    """270 x 480 at R = 150: every window is clipped vertically"""
    ctx = _ctx(gpu_ctx_factory)
    geo, _ = _setup(ctx, SCENE, seed=5)
    assert geo["pixels"] > 0.2 * SCENE[0] * SCENE[1]
    with np.errstate(invalid="ignore"):
        assert (np.abs(geo["xyz_cam"][geo["index"] >= 0]) >= 64).any()  # CW4's exclusion is exercised
    ctx.upload_mask(1, scene_masks[kind])
    got = _compare(ctx, 1, scene_masks[kind], geo, 0, 150)
    assert got["sites"] > 1000
    if kind != "corner":
        assert got["widths"] > 0.5 * got["sites"]


def test_prefix_sums_past_2_to_64(gpu_ctx_factory):
    """1536 x 1536, a point on (nearly) every pixel of a wall at z = 60-63 m: the tables' prefixes wrap"""
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    side = 1536
    shape = (side, side)
    cam = ref.camera(shape)
    px, py = np.meshgrid(np.arange(side), np.arange(side))
    x, y, ok = ref.rays(cam, np.stack([2 * px.ravel(), 2 * py.ravel()], axis=1))  # the rays through the pixel centres
    assert ok.all()
    z = np.random.default_rng(3).uniform(60.0, 63.0, side * side)
    _, c2w = capi.pose_to_matrices(ref.IDENTITY_POSE)
    m = np.asarray(c2w, np.float64).reshape(3, 4)
    cloud = (np.stack([x * z, y * z, z], axis=1) @ m[:, :3].T + m[:, 3]).astype(np.float32)
    geo, _ = _setup(ctx, shape, cloud=cloud)
    member, q = ref.members(geo["index"], geo["xyz_cam"])
    assert geo["pixels"] >= 0.99 * side * side and member.sum() == geo["pixels"]
    assert float((q[..., 2].astype(np.float64) ** 2).sum()) > 2.0 ** 64
    mask = edt_ref.random_mask(shape, 0.5, seed=21)
    ctx.upload_mask(0, mask)
    got = ctx.crack_width(0, 0, 150, want=("flags", "edges", "w2d2", "moments"))
    host = capi.crack_width_host(mask, geo["index"], geo["xyz_cam"], 0, 150)
    assert np.array_equal(got["flags"] & ref.INTEGER_BITS, host["flags"]) and np.array_equal(got["edges"], host["edges"])
    assert np.array_equal(got["w2d2"], host["w2d2"]) and np.array_equal(got["moments"], host["moments"])
    ys, xs = np.nonzero(got["flags"] & ref.SITE)
    pick = np.sort(np.random.default_rng(64).choice(len(ys), 512, replace=False))
    ys, xs = ys[pick], xs[pick]
    assert np.array_equal(got["moments"][ys, xs], ref.moments_at(member, q, ys, xs, 150))


def test_float_stage_against_the_fp64_twin(gpu_ctx_factory, scene_masks):
    """Flags bits 4-6, normal, width and points against the twin (eigh, fp64) at the sites with both edges whose plane is well
    conditioned by the twin's own numbers: n >= 3, eigen-gap (l1 - l0) / trace > 1e-3, incidence >= 0.2 on both rays.  Gates:
    normal 1e-4 per component (the project's gate for smallest_eigenpair against eigh); width relative 2 sqrt(3) 1e-4 / cos_min,
    what that gate implies to first order; points the same relative to |X| plus one fp32 ulp."""
    ctx = _ctx(gpu_ctx_factory)
    geo, _ = _setup(ctx, SCENE, seed=5)
    mask = scene_masks["cracks"]
    ctx.upload_mask(0, mask)
    got = ctx.crack_width(0, 0, 150, want=ALL)
    host = _capi().crack_width_host(mask, geo["index"], geo["xyz_cam"], 0, 150)
    assert np.array_equal(got["moments"], host["moments"]) and np.array_equal(got["edges"], host["edges"])
    both = (got["flags"] & (ref.NEAR | ref.FAR)) == (ref.NEAR | ref.FAR)
    ys, xs = np.nonzero(both)
    twin = ref.float_stage(ref.camera(SCENE), host["moments"][ys, xs], host["edges"][ys, xs])
    keep = twin["plane_ok"] & (twin["gap"] > 1e-3) & (twin["cos"] >= 0.2)
    assert len(ys) > 1000 and keep.sum() >= 0.9 * len(ys), "the scene is wrong: too few well-conditioned sites"
    ys, xs = ys[keep], xs[keep]
    twin = {k: v[keep] for k, v in twin.items()}
    f = got["flags"][ys, xs]
    assert ((f & ref.PLANE) != 0).all()
    assert np.array_equal((f & ref.RAYS) != 0, twin["rays_ok"]) and np.array_equal((f & ref.WIDTH) != 0, twin["rays_ok"])
    assert twin["rays_ok"].sum() >= 0.9 * len(ys)
    plane = got["plane"][ys, xs].astype(np.float64)
    n_err = np.abs(plane[:, :3] - twin["normal"]).max()
    d_err = np.abs(plane[:, 3] - twin["offset"]).max()
    ok = twin["rays_ok"]
    cos_min = float(twin["cos"][ok].min())
    bound = 2.0 * np.sqrt(3.0) * 1e-4 / cos_min
    w_got, w_want = got["width"][ys, xs].astype(np.float64)[ok], twin["width"][ok]
    w_err = (np.abs(w_got - w_want) / w_want).max()
    pts = got["points"][ys, xs].astype(np.float64)[ok]
    want_pts = np.concatenate([twin["near"][ok], twin["far"][ok]], axis=1)
    norms = np.concatenate([np.repeat(np.linalg.norm(twin["near"][ok], axis=1)[:, None], 3, 1),
                            np.repeat(np.linalg.norm(twin["far"][ok], axis=1)[:, None], 3, 1)], axis=1)
    p_err = (np.abs(pts - want_pts) / norms).max()
    print(f"crack width float stage: {len(ys)} sites, {int(ok.sum())} widths, cos_min {cos_min:.4f}, normal {n_err:.3e}, offset {d_err:.3e} m, "
          f"width rel {w_err:.3e} (bound {bound:.3e}), points rel {p_err:.3e}, median width {np.median(w_want) * 1e3:.3f} mm")
    assert n_err <= 1e-4
    assert w_err <= bound
    ulp = np.spacing(np.abs(want_pts).astype(np.float32)).astype(np.float64)
    assert (np.abs(pts - want_pts) <= bound * norms + ulp).all()


def test_same_bytes_twice_and_after_a_permuted_upload(gpu_ctx_factory, scene_masks):
    ctx = _ctx(gpu_ctx_factory)
    geo, cloud = _setup(ctx, SCENE, seed=5)
    ctx.upload_mask(3, scene_masks["cracks"])
    a = ctx.crack_width(3, 0, 150, want=ALL)
    b = ctx.crack_width(3, 0, 150, want=ALL)
    perm = np.random.default_rng(8).permutation(len(cloud))
    ctx.upload_cloud(cloud[perm, 0].copy(), cloud[perm, 1].copy(), cloud[perm, 2].copy())
    c = ctx.crack_width(3, 0, 150, want=ALL)
    for k in ALL:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    assert a["widths"] == b["widths"] == c["widths"] > 0


def test_state_rules_and_error_returns(gpu_ctx_factory):
    capi = _capi()
    C = capi.C

    def code(fn, *a, **kw):
        with pytest.raises(capi.PcpError) as e:
            fn(*a, **kw)
        return e.value.code, str(e.value)

    fresh = gpu_ctx_factory()
    assert code(fresh.crack_width, 0)[0] == capi.PCP_ERR_STATE  # no camera
    fresh.set_camera(cam_struct(capi, ref.camera((9, 11))), _cull(capi))
    rc, msg = code(fresh.crack_width, 0)
    assert rc == capi.PCP_ERR_STATE and "cloud" in msg
    fresh.upload_cloud(np.zeros(4, np.float32), np.zeros(4, np.float32), np.ones(4, np.float32))
    assert code(fresh.crack_width, 0)[0] == capi.PCP_ERR_STATE  # no keyframes
    fresh.set_frames(np.tile(ref.IDENTITY_POSE, (2, 1)))
    rc, msg = code(fresh.crack_width, 0)
    assert rc == capi.PCP_ERR_STATE and "pcp_upload_mask" in msg  # no mask
    fresh.upload_image(1, np.zeros((9, 11, 3), np.uint8))
    assert code(fresh.crack_width, 1)[0] == capi.PCP_ERR_STATE  # an image, but no mask
    fresh.upload_mask(0, np.full((9, 11), 255, np.uint8))
    out = fresh.crack_width(0)
    assert out["flags"].shape == (9, 11) and (out["flags"] == ref.SITE).all() and out["sites"] == 99 and out["widths"] == 0
    assert code(fresh.crack_width, 2)[0] == capi.PCP_ERR_RANGE and code(fresh.crack_width, -1)[0] == capi.PCP_ERR_RANGE
    for t, r in ((-1, 150), (256, 150), (0, 0), (0, 182)):
        assert code(fresh.crack_width, 0, t, r)[0] == capi.PCP_ERR_INVALID, (t, r)
    assert fresh.lib.pcp_crack_width(fresh.h, C.c_int32(0), None, None, None, None, None, None, None, None, None, None) == capi.PCP_ERR_INVALID
    prm = capi.CrackParams(0, 150)
    assert fresh.lib.pcp_crack_width(fresh.h, C.c_int32(0), C.byref(prm), None, None, None, None, None, None, None, None, None) == capi.PCP_OK
    with pytest.raises(ValueError):
        fresh.crack_width(0, want=("flags", "skeleton"))
    fresh.set_camera(cam_struct(capi, ref.camera((1, 16385))), _cull(capi))
    fresh.upload_mask(0, np.zeros((1, 16385), np.uint8))
    rc, msg = code(fresh.crack_width, 0)
    assert rc == capi.PCP_ERR_RANGE and "16384" in msg


def test_nothing_else_moves(gpu_ctx_factory, small_scene):
    """the texels, a colour run, pcp_frame_visible and later pcp_mask_edt / pcp_frame_geometry results are as without the call"""
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
    bgr0, mask0 = ctx.download_image(2)
    vis0 = ctx.frame_visible(2)
    edt0 = ctx.mask_edt(2, 100)
    geo0 = ctx.frame_geometry(2, normals=False)
    out = ctx.crack_width(2, 0, 150)
    assert out["sites"] == int((s["masks"][2] > 0).sum()) and out["widths"] > 0
    ctx.crack_width(4, 100, 20, want=("width",))
    assert np.array_equal(ctx.download_result_packed(), packed)  # the colour result in place
    bgr1, mask1 = ctx.download_image(2)
    assert bgr0.tobytes() == bgr1.tobytes() and mask0.tobytes() == mask1.tobytes()
    vis1 = ctx.frame_visible(2)
    assert all(np.array_equal(vis0[k], vis1[k]) for k in vis0)
    edt1 = ctx.mask_edt(2, 100)
    assert all(np.array_equal(edt0[k], edt1[k]) for k in edt0)
    geo1 = ctx.frame_geometry(2, normals=False)
    assert all(np.array_equal(geo0[k], geo1[k]) for k in geo0)
    after = ctx.colorize()
    assert before["rgb"].tobytes() == after["rgb"].tobytes() and before["has"].tobytes() == after["has"].tobytes()
    # and the call is the host form of that keyframe's own maps
    host = capi.crack_width_host(s["masks"][2], geo0["index"], geo0["xyz_cam"], 0, 150)
    assert np.array_equal(out["flags"] & ref.INTEGER_BITS, host["flags"]) and np.array_equal(out["edges"], host["edges"])
