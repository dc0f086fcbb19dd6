"""The geometry maps on the device ("Geometry maps") against _geometry_ref.py: the moments of the map normals
bit for bit, the normals against numpy's eigh of the same covariance, and the per-pixel maps bit for bit against the
reduction of what pcp_frame_visible and pcp_project_frame report (both pinned to the oracle by their own suites)."""
import numpy as np
import pytest

import _geometry_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

RADII = (0.3, 0.5, 1.0)
AWAY = np.array([0.0, 0.0, 100.0, 1.0, 0.0, 0.0, 0.0])  # above the room, looking further up: sees nothing


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


def _xyz(s):
    return np.stack([s["x"], s["y"], s["z"]], axis=1)


def _context(make, s, cull_mode, xyz=None, images=False, cam=None):
    capi = _capi()
    ctx = make()
    cull = capi.default_cull_params()
    cull.cull_mode = cull_mode
    ctx.set_camera(cam_struct(capi, cam or s["cam"]), cull)
    xyz = _xyz(s) if xyz is None else xyz
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    ctx.set_frames(np.concatenate([s["poses"], AWAY[None]]))
    if images:
        for f, (im, mk) in enumerate(zip(s["images"], s["masks"])):
            ctx.upload_image(f, im)
            ctx.upload_mask(f, mk)
        away = len(s["poses"])  # (the whole-run calls want an image for every keyframe)
        ctx.upload_image(away, np.zeros_like(s["images"][0]))
        ctx.upload_mask(away, np.zeros_like(s["masks"][0]))
    return ctx


# the twin's moments and normals of small_scene per radius and one z-buffer context with its images: computed once, shared;
# every test uploads the cloud it needs
_BASE = {}


def _base(make, s):
    if not _BASE:
        xyz = _xyz(s)
        mom = {r: ref.moments(r, xyz) for r in RADII}
        twin = {r: ref.normals(mom[r]) for r in RADII}
        for r in RADII:
            mom[r].setflags(write=False)
        ctx = _context(make, s, _capi().CULL_ZBUFFER, images=True)
        _BASE.update(xyz=xyz, mom=mom, twin=twin, ctx=ctx)
    return _BASE


@pytest.mark.parametrize("radius", RADII)
def test_moments_exact(gpu_ctx_factory, small_scene, radius):
    b = _base(gpu_ctx_factory, small_scene)
    ctx = b["ctx"]
    ctx.upload_cloud(small_scene["x"], small_scene["y"], small_scene["z"])
    valid, got = ctx.estimate_normals(radius, want_moments=True)
    assert np.array_equal(got, b["mom"][radius])
    assert valid == int(b["twin"][radius]["valid"].sum())
    assert np.array_equal(ctx.normals_fetch()["neighbours"], got[:, 0].astype(np.int32))


@pytest.mark.parametrize("radius", RADII)
def test_moments_exact_with_duplicates_and_non_finite_points(gpu_ctx_factory, small_scene, radius):
    b = _base(gpu_ctx_factory, small_scene)
    ctx = b["ctx"]
    xyz = ref.dirty_cloud(b["xyz"])
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    _, got = ctx.estimate_normals(radius, want_moments=True)
    assert np.array_equal(got, ref.moments(radius, xyz))
    bad = ~np.isfinite(xyz).all(axis=1)
    out = ctx.normals_fetch()
    assert bad.sum() == 2 and not out["normal"][bad].any() and not out["curvature"][bad].any() and not out["neighbours"][bad].any()


def test_all_duplicate_cloud_is_one_cell_and_invalid(gpu_ctx_factory, small_scene):
    ctx = _base(gpu_ctx_factory, small_scene)["ctx"]
    xyz = np.tile(np.array([1.25, -2.5, 0.75], np.float32), (3000, 1))
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    valid, got = ctx.estimate_normals(0.3, want_moments=True)
    assert (got[:, 0] == 3000).all() and not got[:, 1:].any()  # S1 = S2 = 0
    out = ctx.normals_fetch()
    assert valid == 0 and not out["normal"].any() and not out["curvature"].any() and (out["neighbours"] == 3000).all()


def test_all_non_finite_cloud(gpu_ctx_factory, small_scene):
    ctx = _base(gpu_ctx_factory, small_scene)["ctx"]
    xyz = np.ones((10, 3), np.float32)
    xyz[:, 0] = np.nan
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    valid, got = ctx.estimate_normals(0.3, want_moments=True)
    out = ctx.normals_fetch()
    assert valid == 0 and not got.any()
    assert not out["normal"].any() and not out["curvature"].any() and not out["neighbours"].any()


def test_one_cell_of_65_finite_points_and_a_nan(gpu_ctx_factory, small_scene):
    """one full work item of 64 queries plus one, through the gathered view of the finite points"""
    ctx = _base(gpu_ctx_factory, small_scene)["ctx"]
    rng = np.random.default_rng(65)
    xyz = np.float32([1.0, -2.0, 0.5]) + rng.random((66, 3)).astype(np.float32) * np.float32(0.05)
    xyz[40, 1] = np.nan
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    valid, got = ctx.estimate_normals(0.3, want_moments=True)
    mom = ref.moments(0.3, xyz)
    twin = ref.normals(mom)
    assert np.array_equal(got, mom) and (mom[np.arange(66) != 40, 0] == 65).all() and not got[40].any()
    assert valid == int(twin["valid"].sum()) == 65
    out = ctx.normals_fetch()
    assert np.array_equal(out["neighbours"], mom[:, 0].astype(np.int32))
    assert np.array_equal(out["normal"].any(axis=1), twin["valid"])
    n = out["normal"][twin["valid"]].astype(np.float64)
    t = twin["normal"][twin["valid"]]
    assert np.abs(n - t * np.sign((n * t).sum(axis=1))[:, None]).max() <= 1e-4  # (the bar of test_normals_against_eigh)


def test_order_independence(gpu_ctx_factory, small_scene):
    b = _base(gpu_ctx_factory, small_scene)
    ctx, xyz = b["ctx"], b["xyz"]
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    ctx.estimate_normals(0.5)
    first = ctx.normals_fetch()
    p = np.random.default_rng(9).permutation(len(xyz))
    q = xyz[p]
    ctx.upload_cloud(q[:, 0], q[:, 1], q[:, 2])
    ctx.estimate_normals(0.5)
    again = ctx.normals_fetch()
    for k in ("normal", "curvature", "neighbours"):
        assert again[k].tobytes() == first[k][p].tobytes(), k


@pytest.mark.parametrize("radius", RADII)
def test_normals_against_eigh(gpu_ctx_factory, small_scene, radius):
    b = _base(gpu_ctx_factory, small_scene)
    ctx, xyz, twin = b["ctx"], b["xyz"], b["twin"][radius]
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    ctx.estimate_normals(radius)
    got = ctx.normals_fetch()
    valid = got["normal"].any(axis=1)
    assert np.array_equal(valid, twin["valid"])  # invalid points are exactly the twin's
    assert not got["curvature"][~valid].any()
    exempt = twin["valid"] & (twin["gap"] < 1e-3)
    print("radius", radius, "smallest eigen-gap", float(twin["gap"][twin["valid"]].min()), "exempt", int(exempt.sum()))
    assert int(exempt.sum()) == 0  # the reference alone exempts none on this scene (allowed: 1 % of the points)
    check = valid & ~exempt
    n = got["normal"][check].astype(np.float64)
    t = twin["normal"][check]
    t = t * np.sign((n * t).sum(axis=1))[:, None]  # the sign of the world normal is unspecified
    err = np.abs(n - t).max()
    c, ct = got["curvature"][check].astype(np.float64), twin["curvature"][check]
    cerr = np.abs(c - ct)
    print("largest component error", float(err), "largest curvature error", float(cerr.max()), "relative",
          float((cerr / np.maximum(np.abs(ct), 1e-300)).max()))
    assert err <= 1e-4
    assert ((cerr <= 1e-4 * np.abs(ct)) | (cerr <= 1e-9)).all()
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-6


def _reference_maps(ctx, frame):
    cam = ctx.camera
    vis = ctx.frame_visible(frame)
    prj = ctx.project_frame(frame, want_pixel=True, want_cam=False)
    idx = vis["index"]
    assert (prj["pixel"][idx] >= 0).all()  # GM1: every contributor has a colour pixel
    return ref.reduce_maps(cam.image_width, cam.image_height, idx, prj["pixel"][idx], prj["range"][idx], vis["xyz_cam"]), vis


def _assert_maps_equal(ctx, frame, want):
    got = ctx.frame_geometry(frame, normals=False)
    assert got["index"].tobytes() == want["index"].tobytes()
    assert got["range"].tobytes() == want["range"].tobytes()
    assert got["xyz_cam"].tobytes() == want["xyz_cam"].tobytes()
    assert got["pixels"] == want["pixels"] == int((got["index"] >= 0).sum())
    return got


@pytest.mark.parametrize("mode", ("CULL_ZBUFFER", "CULL_HPR"))
def test_maps_exact(gpu_ctx_factory, small_scene, mode):
    s = small_scene
    capi = _capi()
    ctx = _base(gpu_ctx_factory, s)["ctx"] if mode == "CULL_ZBUFFER" else _context(gpu_ctx_factory, s, capi.CULL_HPR)
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    total = 0
    for f in range(len(s["poses"])):
        want, _ = _reference_maps(ctx, f)
        _assert_maps_equal(ctx, f, want)
        total += want["pixels"]
    assert total > 1000
    away = len(s["poses"])
    assert ctx.frame_visible(away)["count"] == 0
    got = ctx.frame_geometry(away, normals=False)
    assert got["pixels"] == 0 and (got["index"] == -1).all() and not got["range"].any() and not got["xyz_cam"].any()


def _pinhole_winners(cam, pose, xyz):
    """Undistorted pinhole estimate of the nearest point per pixel of one keyframe: their indices and the crowded pixels."""
    w2c = _capi().pose_to_matrices(pose)[0].reshape(3, 4).astype(np.float64)
    pc = xyz.astype(np.float64) @ w2c[:, :3].T + w2c[:, 3]
    z = pc[:, 2]
    ok = z > 0
    u = np.where(ok, cam["fx"] * pc[:, 0] / np.where(ok, z, 1.0) + cam["cx"], -1.0)
    v = np.where(ok, cam["fy"] * pc[:, 1] / np.where(ok, z, 1.0) + cam["cy"], -1.0)
    ok &= (u >= 0) & (u < cam["image_width"]) & (v >= 0) & (v < cam["image_height"])
    idx = np.flatnonzero(ok)
    pix = v[idx].astype(np.int64) * cam["image_width"] + u[idx].astype(np.int64)
    rng = np.linalg.norm(pc[idx], axis=1)
    order = np.lexsort((rng, pix))
    first = np.flatnonzero(np.concatenate([[True], pix[order][1:] != pix[order][:-1]]))
    counts = np.diff(np.concatenate([first, [len(order)]]))
    return idx[order[first]], int((counts >= 2).sum())


def test_collisions_and_ties(gpu_ctx_factory, small_scene):
    """200 000 points on a 160 x 90 image: many contributors per pixel, and 200 exact copies whose originals the pinhole
    estimate sees nearest in their pixel (keyframes 0 and 3), so that copy and original tie on range as the two best."""
    from pointcloudprocessor_amd import synth

    s = small_scene
    capi = _capi()
    cam = dict(s["cam"], fx=564.625 / 3, fy=564.625 / 3, cx=80.0, cy=45.0, image_width=160, image_height=90, cull_width=160, cull_height=90)
    x, y, z, _ = synth.make_cloud(200000)
    xyz = np.stack([x, y, z], axis=1)
    rng = np.random.default_rng(77)
    picks = []
    for f in (0, 3):
        win, crowded = _pinhole_winners(cam, s["poses"][f], xyz)
        print("keyframe", f, "pinhole estimate: pixels with two contributors or more", crowded)
        picks.append(rng.choice(win, 100, replace=False))
    xyz = np.concatenate([xyz, xyz[np.concatenate(picks)]])
    for mode in (capi.CULL_HPR_CANDIDATES, capi.CULL_ZBUFFER):
        ctx = _context(gpu_ctx_factory, s, mode, xyz=xyz, cam=cam)
        crowded, tied, ties_to_lower = [], 0, 0
        for f in range(len(s["poses"])):
            want, vis = _reference_maps(ctx, f)
            crowded.append(want["crowded"])
            tied += want["tied"]
            got = _assert_maps_equal(ctx, f, want)
            # a copy (index >= 200 000) never wins against its original
            ties_to_lower += int((got["index"] >= 200000).sum())
        print("mode", mode, "pixels with two contributors or more per keyframe", crowded, "pixels whose two best tie", tied)
        if mode == capi.CULL_HPR_CANDIDATES:
            assert max(crowded) >= 500
        assert tied >= 20
        assert ties_to_lower == 0
        ctx.close()


def test_normal_map(gpu_ctx_factory, small_scene):
    s = small_scene
    capi = _capi()
    b = _base(gpu_ctx_factory, s)
    ctx = b["ctx"]
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    with pytest.raises(capi.PcpError) as e:  # GM5: no estimate on this cloud
        ctx.frame_geometry(0)
    assert e.value.code == capi.PCP_ERR_STATE and "pcp_estimate_normals" in str(e.value)
    with pytest.raises(capi.PcpError) as e:
        ctx.normals_fetch()
    assert e.value.code == capi.PCP_ERR_STATE
    ctx.estimate_normals(0.5)
    nrm = ctx.normals_fetch()["normal"]
    occupied = exempt = 0
    for f in range(len(s["poses"])):
        got = ctx.frame_geometry(f)
        plain = ctx.frame_geometry(f, normals=False)
        for k in ("index", "range", "xyz_cam"):
            assert got[k].tobytes() == plain[k].tobytes(), k
        hit = got["index"] >= 0
        assert not got["normal_cam"][~hit].any()
        w2c = capi.pose_to_matrices(s["poses"][f])[0].reshape(3, 4)
        pc = got["xyz_cam"][hit].astype(np.float64)
        want = ref.normal_cam(w2c, nrm[got["index"][hit]], pc)
        have = got["normal_cam"][hit].astype(np.float64)
        grazing = np.abs((want * pc).sum(axis=1)) <= 1e-5 * np.linalg.norm(pc, axis=1)
        want[grazing] *= np.sign((want[grazing] * have[grazing]).sum(axis=1))[:, None]  # the sign is free only there
        assert np.abs(have - want).max() <= 1e-6
        assert ((have * pc).sum(axis=1) <= 1e-5 * np.linalg.norm(pc, axis=1)).all()  # faces the camera
        occupied += int(hit.sum())
        exempt += int(grazing.sum())
    print("occupied pixels", occupied, "grazing (sign exempt)", exempt)
    assert occupied > 1000 and exempt <= 0.001 * occupied
    ctx.upload_cloud(s["x"], s["y"], s["z"])  # a new cloud drops the estimate
    with pytest.raises(capi.PcpError) as e:
        ctx.frame_geometry(0)
    assert e.value.code == capi.PCP_ERR_STATE
    assert ctx.frame_geometry(0, normals=False)["pixels"] > 0


def test_nothing_else_moves(gpu_ctx_factory, small_scene):
    s = small_scene
    b = _base(gpu_ctx_factory, s)
    ctx = b["ctx"]
    F = len(s["poses"])

    def snapshot():
        ctx.upload_cloud(s["x"], s["y"], s["z"])
        ctx.set_label_fusion(True)
        return ctx.colorize(), ctx.colour_labels()

    def per_frame():
        out = []
        for f in range(F):
            vis = ctx.frame_visible(f)
            keep, dmap, kept = ctx.cull_frame(f)
            out.append((vis, keep, dmap, kept))
        return out

    col0, lab0 = snapshot()
    frames0 = per_frame()
    ctx.estimate_normals(0.3)
    for f in range(F):
        ctx.frame_geometry(f)
    frames1 = per_frame()
    for (v0, k0, d0, n0), (v1, k1, d1, n1) in zip(frames0, frames1):
        for k in ("index", "rgb", "mask", "xyz_cam", "xyz_world"):
            assert v0[k].tobytes() == v1[k].tobytes(), k
        assert k0.tobytes() == k1.tobytes() and d0.tobytes() == d1.tobytes() and n0 == n1 and v0["count"] == v1["count"]
    packed = ctx.download_result_packed().copy()
    ctx.estimate_normals(0.5)
    ctx.frame_geometry(2)
    assert np.array_equal(ctx.download_result_packed(), packed)  # the colour result in place is untouched
    col1, lab1 = snapshot()
    assert col0["rgb"].tobytes() == col1["rgb"].tobytes() and col0["has"].tobytes() == col1["has"].tobytes()
    for k in ("label", "hits", "views"):
        assert lab0[k].tobytes() == lab1[k].tobytes(), k
    ctx.upload_cloud(s["x"], s["y"], s["z"])  # (the shared context goes back as it came)
    ctx.set_label_fusion(False)


def test_pipeline_geometry_maps(small_scene):
    """pipeline.PointCloudColorizer.geometry_maps: the library's maps, the normals estimated once per upload and radius."""
    from pointcloudprocessor_amd import pipeline

    s = small_scene
    capi = _capi()
    eng = pipeline.HipEngine(0)
    try:
        eng.configure(cam_struct(capi, s["cam"]), capi.default_cull_params())
        eng.upload_cloud(s["x"], s["y"], s["z"])
        eng.ctx.set_frames(s["poses"])
        col = pipeline.PointCloudColorizer(eng)
        got = col.geometry_maps(1, normal_radius=0.5)
        assert eng.ctx.normals_radius == 0.5
        want = eng.ctx.frame_geometry(1)
        for k in ("index", "range", "xyz_cam", "normal_cam"):
            assert got[k].tobytes() == want[k].tobytes(), k
        assert got["pixels"] == want["pixels"] > 100 and got["normal_cam"].any()
        bare = col.geometry_maps(1, normal_radius=0)
        assert "normal_cam" not in bare and bare["index"].tobytes() == want["index"].tobytes()
        eng.upload_cloud(s["x"], s["y"], s["z"])  # a new upload: the next call estimates again
        assert eng.ctx.normals_radius is None
        again = col.geometry_maps(1, normal_radius=0.5)
        assert again["normal_cam"].tobytes() == want["normal_cam"].tobytes()
    finally:
        eng.close()
