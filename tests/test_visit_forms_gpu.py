"""The short forms of a (tile, keyframe) visit (csrc/pcp_visit_forms.hpp) against the written ones.

Part one, pcp_selftest_visit_forms on the device: the distortion with its doublings folded into FMAs on 2^24 random float
triples per coefficient set, the cell rule on every fp32 quotient bit pattern per axis and the distance score's square root on
every fp32 bit pattern -- zero disagreements each.

Part two, parity with the oracle on a scene that reaches the cell rule's edges: a cull size of 703 x 405 at ds = 14 has a
50 x 28 map that ends at 700 x 392, so quotients in [50, 703 / 14) pass the reference's test against the full cull size and
must still be rejected; points are seeded around all four borders of several keyframes.  project_frame, cull_frame and
colorize must equal the oracle's bit for bit, depth buffer on and off.
"""
import numpy as np
import pytest

from conftest import cam_struct

pytestmark = pytest.mark.gpu

CULL_W, CULL_H, DS = 703, 405, 14
FRAMES = 8


def _camera_dict():
    from pointcloudprocessor_amd import synth

    d = dict(fx=600.0, fy=600.0, cx=351.5, cy=202.5)
    d.update(synth.REF_D)
    d.update(image_width=CULL_W, image_height=CULL_H, cull_width=CULL_W, cull_height=CULL_H)
    return d


def build_scene():
    """40 000 points of the synthetic room and 9 600 seeded through the borders of every keyframe's map: 49 600 points."""
    from pointcloudprocessor_amd import capi, synth

    cd = _camera_dict()
    x, y, z, _ = synth.make_cloud(40000)
    poses, _ = synth.make_trajectory(FRAMES)
    rng = np.random.default_rng(20251018)
    sx, sy, sz = [], [], []
    per = 300
    for pose in poses:
        _, c2w = capi.pose_to_matrices(pose)
        m = np.asarray(c2w, np.float64).reshape(3, 4)
        # pixel bands around the left / right and top / bottom borders of the map and of the cull size (the distortion moves a
        # border pixel by a few pixels: the bands are wide enough to straddle every edge)
        bands = [((-24.0, 10.0), (-20.0, CULL_H + 20.0)), ((680.0, 714.0), (-20.0, CULL_H + 20.0)),
                 ((-20.0, CULL_W + 20.0), (-24.0, 10.0)), ((-20.0, CULL_W + 20.0), (372.0, 416.0))]
        for (u0, u1), (v0, v1) in bands:
            u = rng.uniform(u0, u1, per)
            v = rng.uniform(v0, v1, per)
            d = rng.uniform(1.0, 4.0, per)
            pc = np.stack([(u - cd["cx"]) / cd["fx"] * d, (v - cd["cy"]) / cd["fy"] * d, d, np.ones(per)])
            pw = m @ pc
            sx.append(pw[0])
            sy.append(pw[1])
            sz.append(pw[2])
    x = np.concatenate([x] + sx).astype(np.float32)
    y = np.concatenate([y] + sy).astype(np.float32)
    z = np.concatenate([z] + sz).astype(np.float32)
    images = [synth.make_image(f, CULL_W, CULL_H) for f in range(FRAMES)]
    return dict(cam=cd, x=x, y=y, z=z, poses=poses, images=images)


def edge_counts(scene):
    """From the oracle's own projection (numpy, fp64 as written): per keyframe, the points whose quotient lies in
    [m, cull / ds) on an axis, in (-1, 0) on an axis, and that land in the last column or row of the map."""
    from oracle import np_oracle, oracle_capi

    cd = scene["cam"]
    mw, mh = CULL_W // DS, CULL_H // DS
    f32 = np.float32
    out = []
    for pose in scene["poses"]:
        w2c, _ = oracle_capi.pose_to_matrices(pose)
        p = np_oracle.project_frame(cd, w2c, scene["x"], scene["y"], scene["z"], ds=DS)
        front = p["zc"] > 0
        with np.errstate(all="ignore"):
            qx = p["u"].astype(f32) / f32(DS)
            qy = p["v"].astype(f32) / f32(DS)
        in_x = (qx > -1) & (qx < f32(mw))
        in_y = (qy > -1) & (qy < f32(mh))
        band = front & (((qx >= f32(mw)) & (qx < f32(CULL_W) / f32(DS)) & in_y) | ((qy >= f32(mh)) & (qy < f32(CULL_H) / f32(DS)) & in_x))
        below = front & (((qx > -1) & (qx < 0) & in_y) | ((qy > -1) & (qy < 0) & in_x))
        cell = p["cell"]
        last = (cell >= 0) & ((cell % mw == mw - 1) | (cell // mw == mh - 1))
        out.append((int(band.sum()), int(below.sum()), int(last.sum())))
    return out


@pytest.fixture(scope="module")
def edge_scene():
    return build_scene()


COEFFS = {
    "default": None,
    "all_zero": dict(k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0),
    "radial_only": dict(k1=0.1, k2=-0.02, k3=0.003, p1=0.0, p2=0.0),
    "negative_tangential": dict(k1=-0.2, k2=0.05, k3=-0.001, p1=-0.01, p2=-0.02),
    "written_form": dict(p1=1e-200, p2=-0.0006654964142658197),  # p1 below 2^-400: the flag keeps the written form
}


@pytest.mark.parametrize("name", list(COEFFS))
def test_short_distortion_equals_the_written_form(gpu_ctx_factory, name):
    from pointcloudprocessor_amd import capi

    ctx = gpu_ctx_factory()
    cam = capi.default_camera()
    for k, v in (COEFFS[name] or {}).items():
        setattr(cam, k, v)
    ctx.set_camera(cam, capi.default_cull_params())
    bad_uv, _, _, short = ctx.selftest_visit_forms(samples=1 << 24, seed=20251018)
    print(name, "projection mismatches", bad_uv, "short form runs", short)
    assert short == (name != "written_form")
    assert bad_uv == 0
    ctx.close()


@pytest.mark.parametrize("ds", [14, 1, 7, 20])
def test_short_cell_rule_and_square_root_on_every_bit_pattern(gpu_ctx_factory, ds):
    from pointcloudprocessor_amd import capi

    ctx = gpu_ctx_factory()
    cam = capi.default_camera()
    cam.cull_width, cam.cull_height = CULL_W, CULL_H  # not a multiple of any of the factors but 1
    cull = capi.default_cull_params()
    cull.downsample_factor = ds
    ctx.set_camera(cam, cull)
    _, bad_cell, bad_sqrt, _ = ctx.selftest_visit_forms(samples=0)
    print("ds", ds, "cell mismatches", bad_cell, "sqrt mismatches", bad_sqrt)
    assert bad_cell == 0
    assert bad_sqrt == 0
    ctx.close()


def test_the_scene_reaches_the_edges_of_the_cell_rule(edge_scene):
    """(oracle only) a scene that never reaches the edge cases proves nothing"""
    assert len(edge_scene["x"]) <= 50000 and len(edge_scene["poses"]) == FRAMES
    counts = edge_counts(edge_scene)
    print("per keyframe (band, quotient in (-1, 0), last column / row):", counts)
    assert max(c[0] for c in counts) >= 50
    assert max(c[1] for c in counts) >= 50
    assert max(c[2] for c in counts) >= 50


def _setup(ctx, capi, scene, zbuf):
    cull = capi.default_cull_params()
    cull.downsample_factor = DS
    cull.enable_depth_buffer_culling = 1 if zbuf else 0
    ctx.set_camera(cam_struct(capi, scene["cam"]), cull)
    ctx.upload_cloud(scene["x"], scene["y"], scene["z"])
    ctx.set_frames(scene["poses"])
    for f, im in enumerate(scene["images"]):
        ctx.upload_image(f, im)


def _oracle_params(oracle, scene, zbuf):
    ocp = oracle.default_cull_params()
    ocp.downsample_factor = DS
    ocp.enable_depth_buffer_culling = 1 if zbuf else 0
    return cam_struct(oracle, scene["cam"]), ocp


@pytest.mark.parametrize("zbuf", [True, False])
def test_project_and_cull_frame_equal_the_oracle(gpu_ctx_factory, oracle, edge_scene, zbuf):
    from pointcloudprocessor_amd import capi

    s = edge_scene
    ctx = gpu_ctx_factory()
    _setup(ctx, capi, s, zbuf)
    ocam, ocp = _oracle_params(oracle, s, zbuf)
    outside = 0  # candidates without a map cell (-2): only reported with the depth buffer off, the band among them
    for f, pose in enumerate(s["poses"]):
        w2c, _ = oracle.pose_to_matrices(pose)
        ref = oracle.project_frame(ocam, ocp, w2c, s["x"], s["y"], s["z"])
        got = ctx.project_frame(f)
        for k in ("xc", "yc", "zc", "cell", "pixel"):
            assert np.array_equal(got[k], ref[k]), (f, k)
        outside = max(outside, int((ref["cell"] == -2).sum()))
        keep_r, dmap_r, kept_r = oracle.cull_frame(ocam, ocp, w2c, s["x"], s["y"], s["z"])
        keep_g, dmap_g, kept_g = ctx.cull_frame(f)
        if zbuf:
            assert np.array_equal(dmap_g.view(np.uint32), dmap_r.view(np.uint32)), f
        assert np.array_equal(keep_g, keep_r), f
        assert kept_g == kept_r
    assert (outside >= 50) == (not zbuf)
    ctx.close()


@pytest.mark.parametrize("zbuf", [True, False])
def test_colorize_equals_the_oracle(gpu_ctx_factory, oracle, edge_scene, zbuf):
    from pointcloudprocessor_amd import capi

    s = edge_scene
    ctx = gpu_ctx_factory()
    _setup(ctx, capi, s, zbuf)
    ocam, ocp = _oracle_params(oracle, s, zbuf)
    ref = oracle.colorize(ocam, ocp, s["x"], s["y"], s["z"], s["poses"], s["images"])
    assert ref["has"].sum() > 500 and ref["count"].max() >= 3
    ctx.colour_reset()
    ctx.depth_pass()
    ctx.colour_pass()
    got = ctx.colour_finalise(want_top=True)
    for k in ("count", "top_frame", "top_rgb", "rgb", "has"):
        print(k, "differing entries", int((got[k] != ref[k]).sum()))
    print("top_score differing bit patterns", int((got["top_score"].view(np.uint32) != ref["top_score"].view(np.uint32)).sum()))
    for k in ("count", "top_frame", "top_rgb", "rgb", "has"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["top_score"].view(np.uint32), ref["top_score"].view(np.uint32))
    one = ctx.colorize()
    assert np.array_equal(one["rgb"], ref["rgb"]) and np.array_equal(one["has"], ref["has"])
    ctx.close()
