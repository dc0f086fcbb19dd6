"""The crack widths on the map on the device ("Crack widths on the map"): pcp_crack_fuse_* against the library's CPU
form and the restatement in _crack_fuse_ref.py, both fed the device's own per-keyframe inputs -- pcp_crack_width's flags and
width image, pcp_frame_visible's list, pcp_project_frame's pixel and range -- so that this suite pins the reduction and
equality is exact (the float stage of the widths is pinned by its own suite); pcp_crack_components against
pcp_crack_components_host and the restatement under the device's own views; and the fused width of a stripe of known width.

Known stripe, measured on an MI355X (test_known_stripe prints them): w0 50 mm, 348 centre points, worst error 2.484 mm, mean
0.260 mm, bound 16.949 mm (farthest credited range 3.743 m, smallest cosine 0.9201); the fp64 twin of _crack_width_ref.py alone,
on the CPU with a numpy position image of the same scene: worst 2.506 mm over all 12 690 widths."""
import numpy as np
import pytest

import _crack_fuse_ref as ref
import _crack_width_ref as cw_ref
import _mask_edt_ref as edt_ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

SCENE = (270, 480)
FRAMES = 6
RADIUS = 0.005  # of the component cases (test_crack_fuse_cpu.py)
FETCHED = ("width_mean", "width_best", "best_frame", "views", "seen", "centres", "min_q", "max_q", "sum_q")


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


_STATE = {}


def _ctx(make):
    if "ctx" not in _STATE:
        _STATE["ctx"] = make()
    return _STATE["ctx"]


def _setup(ctx, cam, cloud, poses, masks, zbuffer=False):
    capi = _capi()
    cull = capi.default_cull_params()
    cull.enable_depth_buffer_culling = 1 if zbuffer else 0
    ctx.set_camera(cam_struct(capi, cam), cull)  # (drops every uploaded image and mask)
    ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
    ctx.set_frames(np.asarray(poses, np.float64))
    for f, m in enumerate(masks):
        ctx.upload_mask(f, m)


def _inputs(ctx, frames, threshold, radius):
    """per keyframe, from the device's own calls: (index, pixel, range, flags, width)"""
    out = {}
    for f in frames:
        cw = ctx.crack_width(f, threshold, radius, want=("flags", "width"))
        vis = ctx.frame_visible(f)
        assert vis["count"] == len(vis["index"])
        pf = ctx.project_frame(f, want_cam=False)
        index = vis["index"].astype(np.int32)
        assert (pf["pixel"][index] >= 0).all()
        out[f] = (index, pf["pixel"][index], pf["range"][index], cw["flags"], cw["width"])
    return out


def _fuse(ctx, order, threshold, radius):
    ctx.crack_fuse_begin()
    counts = {f: ctx.crack_fuse_add(f, threshold, radius) for f in order}
    return ctx.crack_fuse_fetch(), counts


def _check_fusion(ctx, n, frames, threshold, radius, shuffled):
    """device == host form == restatement; the same bytes for the adds in another order.  Leaves the accumulation live."""
    capi = _capi()
    inp = _inputs(ctx, frames, threshold, radius)
    want, host = ref.new_state(n), capi.crack_fuse_state(n)
    credited = {}
    for f in frames:
        credited[f] = ref.add_frame(want, *inp[f][:3], f, *inp[f][3:])
        assert capi.crack_fuse_host(host, *inp[f][:3], f, *inp[f][3:]) == credited[f]
    for k in ref.FIELDS:
        assert np.array_equal(host[k], want[k]), k
    got_b, _ = _fuse(ctx, shuffled, threshold, radius)
    ctx.crack_fuse_end()
    got, counts = _fuse(ctx, frames, threshold, radius)
    for f in frames:
        assert counts[f] == (len(inp[f][0]), credited[f]), f
    res = ref.results(want)
    for k in FETCHED:
        w = res[k] if k in res else want[k]
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w), k
        assert got[k].tobytes() == got_b[k].tobytes(), k
    return got, want, inp


def _scene_masks(shape, seed):
    m = cw_ref.masks(shape, seed)
    return [m["cracks"], m["half"], edt_ref.crack_mask(shape, seed + 1, cracks=12), m["dense"], edt_ref.crack_mask(shape, seed + 2, cracks=12), m["corner"]]


def _wall(shape, seed):
    _, c2w = _capi().pose_to_matrices(cw_ref.IDENTITY_POSE)
    return cw_ref.wall_cloud(shape, seed=seed, c2w=c2w)


@pytest.mark.parametrize("shape", [(1, 1), (45, 70), (33, 129), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_device_fusion_equals_host_form_and_restatement(gpu_ctx_factory, shape):
    ctx = _ctx(gpu_ctx_factory)
    cloud = _wall(shape, seed=shape[0] * 31 + shape[1])
    _setup(ctx, cw_ref.camera(shape), cloud, ref.fuse_poses(), _scene_masks(shape, seed=shape[0] + 7 * shape[1]))
    got, _, _ = _check_fusion(ctx, len(cloud), list(range(FRAMES)), 0, 7, [4, 1, 5, 0, 3, 2])
    ctx.crack_fuse_end()
    if shape[0] >= 33:
        assert got["views"].max() >= 1


@pytest.fixture(scope="module")
def scene_cloud():
    cloud = _wall(SCENE, seed=5)
    cloud.setflags(write=False)
    return cloud


def test_scene_fusion_at_radius_150_and_its_components(gpu_ctx_factory, scene_cloud):
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    cloud = scene_cloud
    n = len(cloud)
    _setup(ctx, cw_ref.camera(SCENE), cloud, ref.fuse_poses(), _scene_masks(SCENE, seed=4))
    got, want, _ = _check_fusion(ctx, n, list(range(FRAMES)), 0, 150, [3, 0, 5, 2, 1, 4])
    views, seen = got["views"], got["seen"]
    print(f"crack fuse scene: {n} points, credited {(views > 0).sum()}, views >= 3: {(views >= 3).sum()}, seen > views > 0: {((seen > views) & (views > 0)).sum()}")
    assert (views >= 3).any() and ((seen > views) & (views > 0)).any() and (views > 0).sum() > 1000
    first = None
    for radius in (0.02, 0.05):
        for min_views in (3,):  # (the brute-force references are quadratic in the crack points: the few thousand seen three times)
            out = ctx.crack_components(min_views, radius)
            label = out["label"]
            assert np.array_equal(label, capi.crack_components_host(cloud, views, min_views, radius))
            ref.check_labels(label, cloud, views, min_views, radius)
            ids, stats, box = ref.table(label, want, cloud)
            assert np.array_equal(out["ids"], ids) and (np.diff(out["ids"]) > 0).all()
            assert out["stats"].dtype == np.int64 and np.array_equal(out["stats"], stats)
            assert out["box"].dtype == np.float32 and np.array_equal(out["box"], box)
            assert out["components"] == len(ids) and out["crack_points"] == int((label >= 0).sum()) == int(out["stats"][:, 0].sum())
            assert out["components"] > 1
            if first is None:
                first = out
    ctx.crack_fuse_end()
    # a permuted upload: the same partition, every label the lowest NEW index of its members
    perm = np.random.default_rng(8).permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    ctx.upload_cloud(cloud[perm, 0].copy(), cloud[perm, 1].copy(), cloud[perm, 2].copy())
    got2, _ = _fuse(ctx, range(FRAMES), 0, 150)
    for k in FETCHED:
        if k != "best_frame":
            assert np.array_equal(got2[k], got[k][perm]), k
    out2 = ctx.crack_components(3, 0.02)
    ctx.crack_fuse_end()
    assert np.array_equal(out2["label"] >= 0, (first["label"] >= 0)[perm]) and out2["components"] == first["components"]
    lowest = np.full(n, n, np.int64)
    who = np.flatnonzero(first["label"] >= 0)
    np.minimum.at(lowest, first["label"][who], inv[who])
    assert np.array_equal(out2["label"][inv[who]], lowest[first["label"][who]])
    assert np.array_equal(np.sort(out2["stats"], axis=0), np.sort(first["stats"], axis=0))


def test_depth_buffer_culling_contributors_are_the_visible_list(gpu_ctx_factory, scene_cloud):
    """with the depth buffer on, a point hidden in a keyframe is neither seen nor credited there"""
    ctx = _ctx(gpu_ctx_factory)
    far = scene_cloud
    near = (far[far[:, 0] < -0.2] * np.float32(0.5)).astype(np.float32)  # an occluder at half the range in front of the left part
    cloud = np.concatenate([far, near])
    n = len(cloud)
    _setup(ctx, cw_ref.camera(SCENE), cloud, ref.fuse_poses(), _scene_masks(SCENE, seed=4), zbuffer=True)
    got, want, inp = _check_fusion(ctx, n, list(range(FRAMES)), 0, 20, [5, 4, 3, 2, 1, 0])
    ctx.crack_fuse_end()
    listed = np.zeros(n, np.int64)
    projecting = np.zeros(n, np.int64)
    for f in range(FRAMES):
        listed[inp[f][0]] += 1
        projecting += ctx.project_frame(f, want_cam=False)["pixel"] >= 0
    assert np.array_equal(got["seen"], listed)
    hidden = projecting - listed
    assert (hidden >= 0).all() and (hidden > 0).sum() > 1000, "the scene is wrong: the depth buffer hides nothing"
    never = (listed == 0) & (projecting > 0)
    assert never.any() and not got["seen"][never].any() and not got["views"][never].any()


# ---- the component cases of the CPU suite, their views made by synthetic keyframes ------------------------------------------
CASE_SHAPE = (64, 64)


def _case_scene(xyz):
    """The case's points as they are (world = the case's own frame), a camera at the identity rotation backed off along -z so
    that the finite points fill the middle of a 64 x 64 image, and a wall one metre behind them with a point per pixel: the
    wall gives every pixel's window its plane.  Three keyframes of that one pose; the masks have background only in the first
    and last column (keyframe 0: every other pixel gets a width) and, in keyframes 1 and 2, in the right half as well."""
    h, w = CASE_SHAPE
    fin = xyz[np.isfinite(xyz).all(axis=1)]
    lo, hi = fin.min(axis=0).astype(np.float64), fin.max(axis=0).astype(np.float64)
    centre, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    back = max(max(half[0], half[1]) / 0.35, 1.0) + half[2]
    eye = centre - np.array([0.0, 0.0, back])
    depth = back + half[2] + 1.0
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    wall = np.stack([(px.ravel() + 0.5 - w / 2.0) / w * depth, (py.ravel() + 0.5 - h / 2.0) / w * depth, np.full(h * w, depth)], axis=1) + eye
    cloud = np.concatenate([xyz, wall.astype(np.float32)]).astype(np.float32)
    pose = np.array([eye[0], eye[1], eye[2], 1.0, 0.0, 0.0, 0.0])
    full = np.full(CASE_SHAPE, 255, np.uint8)
    full[:, 0] = full[:, -1] = 0
    left = full.copy()
    left[:, w // 2:] = 0
    return cloud, np.tile(pose, (3, 1)), [full, left, left]


@pytest.fixture(scope="module")
def cases():
    return ref.component_cases(RADIUS)


@pytest.mark.parametrize("name", ["chain_shuffled", "chain_descending", "chains_touch", "chains_apart", "duplicates", "ring", "one_cell",
                                  "non_finite", "min_views_1", "min_views_3", "single", "no_crack_point", "uniform"])
def test_device_components_on_the_cpu_cases(gpu_ctx_factory, cases, name):
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    xyz, _, min_views = cases[name]
    k = len(xyz)
    cloud, poses, masks = _case_scene(xyz)
    cam = cw_ref.camera(CASE_SHAPE)
    cam.update(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
    _setup(ctx, cam, cloud, poses, masks)
    frames = [] if name == "no_crack_point" else [0, 1, 2]
    got, counts = _fuse(ctx, frames, 0, 150)
    views = got["views"]
    finite = np.isfinite(xyz).all(axis=1)
    if frames:
        assert (views[:k][finite] >= 1).mean() > 0.9, "the scene is wrong: the case's points are not credited"
        assert not views[:k][~finite].any()
    out = ctx.crack_components(min_views, RADIUS)
    label = out["label"]
    assert np.array_equal(label, capi.crack_components_host(cloud, views, min_views, RADIUS))
    ref.check_labels(label, cloud, views, min_views, RADIUS)
    st = dict(sum_q=got["sum_q"], views=views, centres=got["centres"])
    ids, stats, box = ref.table(label, st, cloud)
    assert np.array_equal(out["ids"], ids) and np.array_equal(out["stats"], stats) and np.array_equal(out["box"], box)
    assert out["crack_points"] == int((label >= 0).sum()) and out["components"] == len(ids)
    ctx.crack_fuse_end()
    sizes = np.bincount(label[:k][label[:k] >= 0], minlength=1)
    if name.startswith("chain_"):
        assert sizes.max() == k and (label[:k] == 0).all()  # one crack through all 4 100 points
    elif name == "chains_touch":
        assert (sizes > 0).sum() == 1
    elif name == "chains_apart":
        assert (sizes > 0).sum() == 2
    elif name == "min_views_3":
        assert (views[:k] == 3).any() and (views[:k] == 1).any() and (label[:k][views[:k] < 3] == -1).all()
    elif name == "no_crack_point":
        assert out["components"] == 0 and out["crack_points"] == 0 and (label == -1).all() and len(out["ids"]) == 0
    elif name == "uniform":
        assert (sizes > 0).sum() > 10 and sizes.max() > 100


def test_known_stripe(gpu_ctx_factory):
    """A stripe of known width on a planar wall, six poses at different ranges and incidences: at the crack points with
    centres > 0 the fused mean is within two pixel footprints (range / fx) at the farthest credited range, divided by the
    smallest incidence cosine among the credited views -- one pixel of edge placement per side under CW3's midpoint rule.
    Measured worst error and bound: see DESIGN.md."""
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    sc = ref.stripe_scene()
    c2w = [capi.pose_to_matrices(p)[1] for p in sc["poses"]]
    masks = [ref.stripe_mask(sc, m) for m in c2w]
    assert all((m > 0).sum() > 500 for m in masks)
    _setup(ctx, sc["cam"], sc["cloud"], sc["poses"], masks)
    inp = _inputs(ctx, range(FRAMES), 0, 150)
    got, _ = _fuse(ctx, range(FRAMES), 0, 150)
    ctx.crack_fuse_end()
    far, cos_min = 0.0, 1.0
    for f in range(FRAMES):
        index, pixel, rng, flags, _ = inp[f]
        ok = (flags.ravel()[pixel] & ref.WIDTH) != 0
        assert ok.any(), f
        eye_z = float(np.asarray(c2w[f], np.float64).reshape(3, 4)[2, 3])
        far = max(far, float(rng[ok].max()))
        cos_min = min(cos_min, float(((3.0 - eye_z) / rng[ok].astype(np.float64)).min()))
    bound = 2.0 * (far / sc["cam"]["fx"]) / cos_min
    pick = (got["views"] > 0) & (got["centres"] > 0)
    err = np.abs(got["width_mean"][pick].astype(np.float64) - sc["w0"])
    print(f"known stripe: w0 {sc['w0'] * 1e3:.1f} mm, {int(pick.sum())} centre points, worst error {err.max() * 1e3:.3f} mm, "
          f"mean {err.mean() * 1e3:.3f} mm, bound {bound * 1e3:.3f} mm (farthest range {far:.3f} m, cos_min {cos_min:.4f})")
    # (non-vacuity: the ridge of the stripe is a column of 270 pixels in keyframe 0 alone, at 0.5 map points per pixel)
    assert pick.sum() > 100
    assert err.max() <= bound


def test_state_rules(gpu_ctx_factory):
    capi = _capi()

    def code(fn, *a, **kw):
        with pytest.raises(capi.PcpError) as e:
            fn(*a, **kw)
        return e.value.code

    ctx = gpu_ctx_factory()
    shape = (33, 129)
    cloud = _wall(shape, seed=3)
    for fn in (ctx.crack_fuse_fetch, ctx.crack_components, ctx.crack_fuse_end):
        assert code(fn) == capi.PCP_ERR_STATE
    assert code(ctx.crack_fuse_add, 0) == capi.PCP_ERR_STATE
    _setup(ctx, cw_ref.camera(shape), cloud, ref.fuse_poses(), _scene_masks(shape, seed=1)[:5])  # (keyframe 5 has no mask)
    for fn in (ctx.crack_fuse_fetch, ctx.crack_components, ctx.crack_fuse_end):
        assert code(fn) == capi.PCP_ERR_STATE
    assert code(ctx.crack_fuse_add, 0) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    fresh = ctx.crack_fuse_fetch()
    assert not fresh["views"].any() and (fresh["min_q"] == ref.NO_MIN).all() and (fresh["best_frame"] == -1).all()
    none = ctx.crack_components()
    assert none["components"] == 0 and none["crack_points"] == 0 and (none["label"] == -1).all()
    ctx.crack_fuse_add(1, 0, 7)
    once = ctx.crack_fuse_fetch()
    assert code(ctx.crack_fuse_add, 1, 0, 7) == capi.PCP_ERR_STATE  # CF4: twice
    assert code(ctx.crack_fuse_add, 5, 0, 7) == capi.PCP_ERR_STATE  # no mask
    assert code(ctx.crack_fuse_add, 6, 0, 7) == capi.PCP_ERR_RANGE and code(ctx.crack_fuse_add, -1, 0, 7) == capi.PCP_ERR_RANGE
    for t, r in ((-1, 150), (256, 150), (0, 0), (0, 182)):
        assert code(ctx.crack_fuse_add, 0, t, r) == capi.PCP_ERR_INVALID, (t, r)
    for mv, r in ((0, 0.02), (4097, 0.02), (1, 0.004), (1, 1.5)):
        assert code(ctx.crack_components, mv, r) == capi.PCP_ERR_INVALID, (mv, r)
    again = ctx.crack_fuse_fetch()
    assert all(once[k].tobytes() == again[k].tobytes() for k in once)  # the refused calls changed nothing
    with pytest.raises(ValueError):
        ctx.crack_fuse_fetch(want=("views", "skeleton"))
    assert set(ctx.crack_fuse_fetch(want=("width_mean",))) == {"width_mean"}
    ctx.crack_fuse_add(0, 0, 7)
    # the drops: an upload, the camera, the keyframes
    ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
    assert code(ctx.crack_fuse_fetch) == capi.PCP_ERR_STATE and code(ctx.crack_fuse_add, 2, 0, 7) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    ctx.set_frames(ref.fuse_poses())
    assert code(ctx.crack_fuse_fetch) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    cull = capi.default_cull_params()
    ctx.set_camera(cam_struct(capi, cw_ref.camera(shape)), cull)
    assert code(ctx.crack_components) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    ctx.crack_fuse_end()
    assert code(ctx.crack_fuse_end) == capi.PCP_ERR_STATE


def test_nothing_else_moves(gpu_ctx_factory, small_scene):
    """the texels, a colour run, pcp_frame_visible and later pcp_crack_width / pcp_mask_edt / pcp_frame_geometry results are as
    without a full begin / add / components / end cycle"""
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
    all_outputs = ("flags", "edges", "w2d2", "width", "points", "plane", "moments")
    cw0 = ctx.crack_width(2, 0, 150, want=all_outputs)
    ctx.crack_fuse_begin()
    for f in (3, 2, 0):
        m, c = ctx.crack_fuse_add(f, 0, 150)
        assert m > 0
    state = ctx.crack_fuse_fetch()
    assert (state["views"] > 0).any()
    out = ctx.crack_components(1, 0.05)
    assert out["components"] >= 1
    ctx.crack_fuse_end()
    assert np.array_equal(ctx.download_result_packed(), packed)  # the colour result in place
    bgr1, mask1 = ctx.download_image(2)
    assert bgr0.tobytes() == bgr1.tobytes() and mask0.tobytes() == mask1.tobytes()
    vis1 = ctx.frame_visible(2)
    assert all(np.array_equal(vis0[k], vis1[k]) for k in vis0)
    edt1 = ctx.mask_edt(2, 100)
    assert all(np.array_equal(edt0[k], edt1[k]) for k in edt0)
    geo1 = ctx.frame_geometry(2, normals=False)
    assert all(np.array_equal(geo0[k], geo1[k]) for k in geo0)
    cw1 = ctx.crack_width(2, 0, 150, want=all_outputs)
    for k in all_outputs:
        assert cw0[k].tobytes() == cw1[k].tobytes(), k
    assert (cw0["sites"], cw0["widths"]) == (cw1["sites"], cw1["widths"])
    after = ctx.colorize()
    assert before["rgb"].tobytes() == after["rgb"].tobytes() and before["has"].tobytes() == after["has"].tobytes()
    # and pcp_crack_width is still the host form of that keyframe's own maps
    host = capi.crack_width_host(s["masks"][2], geo0["index"], geo0["xyz_cam"], 0, 150)
    assert np.array_equal(cw1["flags"] & cw_ref.INTEGER_BITS, host["flags"]) and np.array_equal(cw1["edges"], host["edges"])
    assert np.array_equal(cw1["w2d2"], host["w2d2"]) and np.array_equal(cw1["moments"], host["moments"])
