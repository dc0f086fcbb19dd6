"""The batched passes of the default configuration leave the k3 term out of the radial polynomial when the camera's k3 is a zero and
its other constants pass k3_term_droppable (csrc/pcp_visit_forms.hpp); any other camera keeps the term and stays in the default
configuration.

Part one, pcp_selftest_k3_term on the device: the written projection against the form the passes run under the configured camera,
on 2^24 random float triples per coefficient set and on a grid of extreme triples -- zero disagreements in the verdicts of the two
truncation rules, in cell and pixel, and in (u, v) where a rule accepts.

Part two, parity with the oracle at "tiny", 3000 points x 70 keyframes: every depth map, colours and `has`, for k3 = 0.0, k3 = -0.0,
k3 != 0 (term kept) and a coefficient set that fails the host's condition (term kept).

Part three, a second cloud in front of an identity-pose keyframe for case c of the proof (r6 overflows, the written form's
0 * inf = NaN rejects the lane): points at 0 < zc <= 2^-100 with |xc| or |yc| near 1, which the reference rejects (u, v beyond
2^100 px); points at zc <= 2^-140 with |xc| or |yc| between 2^31 and 2^39, the ones whose r6 really overflows (|xc| near 1 over the
smallest fp32 depth, 2^-149, gives r2 = 2^298 and r6 = 2^894, short of 2^1024: xn has to reach 2^171), rejected as well; and points
at xc = yc = 0 with tiny zc, which the reference accepts (they image at (cx, cy)).  The oracle alone must say so before anything is
compared.
"""
import numpy as np
import pytest

from conftest import cam_struct

pytestmark = pytest.mark.gpu

N, F = 3000, 70

# name -> (overrides of the "tiny" camera, the term is dropped)
CAMERAS = {
    "k3_zero": (dict(k3=0.0), True),
    "k3_negative_zero": (dict(k3=-0.0), True),
    "k3_nonzero": (dict(k3=0.003), False),
    "no_leading_coefficient": (dict(k1=0.0, k2=0.0, k3=0.0), False),  # tangential terms only: fails the host's condition
}
# further coefficient sets for the device self-test
SELFTEST = dict(CAMERAS)
SELFTEST.update({
    "no_distortion": (dict(k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0), True),
    "k1_leads": (dict(k1=-0.2, k2=0.0, k3=-0.0, p1=-0.01, p2=-0.02), True),
    "k2_alone": (dict(k1=0.0, k2=0.05, k3=0.0, p1=0.0, p2=0.001), True),
    "edges_of_the_range": (dict(k1=2.0 ** -60, k2=-(2.0 ** 60), k3=0.0, p1=2.0 ** 60, p2=-(2.0 ** -60), fx=2.0 ** -20, fy=2.0 ** 40,
                                cx=2.0 ** 40, cy=-(2.0 ** 40)), True),
    "k1_too_small": (dict(k1=1e-30, k3=0.0), False),
    "fx_too_large": (dict(fx=2.0 ** 41, k3=0.0), False),
})


def camera(overrides):
    from pointcloudprocessor_amd import synth

    cd = synth.camera_dict("tiny")
    cd.update(overrides)
    return cd


@pytest.mark.parametrize("name", list(SELFTEST))
def test_device_selftest_has_no_disagreement(gpu_ctx_factory, name):
    from pointcloudprocessor_amd import capi

    overrides, dropped = SELFTEST[name]
    ctx = gpu_ctx_factory()
    ctx.set_camera(cam_struct(capi, camera(overrides)))
    bad, flag = ctx.selftest_k3_term(samples=1 << 24, seed=20261020)
    print(name, "mismatches", bad, "term dropped", flag)
    assert flag == dropped
    assert bad == 0
    # the existing self-test keeps its meaning: the short distortion WITH the term against the written form
    bad_uv, _, _, _ = ctx.selftest_visit_forms(samples=1 << 20, seed=3)
    assert bad_uv == 0
    ctx.close()


@pytest.fixture(scope="module")
def room():
    from pointcloudprocessor_amd import synth

    x, y, z, _ = synth.make_cloud(N)
    poses, _ = synth.make_trajectory(F)
    four = [synth.make_image(f, 480, 270) for f in range(4)]
    return dict(x=x, y=y, z=z, poses=poses, images=[four[f % 4] for f in range(F)])


def loaded_context(factory, cd, s):
    from pointcloudprocessor_amd import capi

    ctx = factory()
    ctx.set_camera(cam_struct(capi, cd))
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
    return ctx


def compare_with_oracle(ctx, oracle, cd, s):
    """every depth map of the batched pass, then colours and `has` of the whole-run call"""
    ocam, ocp = cam_struct(oracle, cd), oracle.default_cull_params()
    ctx.depth_pass()
    differing = 0
    for f, pose in enumerate(s["poses"]):
        w2c, _ = oracle.pose_to_matrices(pose)
        _, dmap, _ = oracle.cull_frame(ocam, ocp, w2c, s["x"], s["y"], s["z"])
        differing += int((ctx.download_depth_map(f).view(np.uint32) != dmap.view(np.uint32)).sum())
    ref = oracle.colorize(ocam, ocp, s["x"], s["y"], s["z"], s["poses"], s["images"], threads=8, want_top=False)
    got = ctx.colorize()
    staged = ctx.colorize_from_depth()
    print("depth map cells differing", differing, "colours differing", int((got["rgb"] != ref["rgb"]).any(axis=1).sum()),
          "has differing", int((got["has"] != ref["has"]).sum()), "coloured", int(ref["has"].sum()))
    assert differing == 0
    assert np.array_equal(got["rgb"], ref["rgb"]) and np.array_equal(got["has"], ref["has"])
    assert np.array_equal(staged["rgb"], ref["rgb"]) and np.array_equal(staged["has"], ref["has"])
    return ref


@pytest.mark.parametrize("name", list(CAMERAS))
def test_depth_maps_and_colours_equal_the_oracle(gpu_ctx_factory, oracle, room, name):
    overrides, dropped = CAMERAS[name]
    cd = camera(overrides)
    ctx = loaded_context(gpu_ctx_factory, cd, room)
    assert ctx.selftest_k3_term(samples=0)[1] == dropped
    ref = compare_with_oracle(ctx, oracle, cd, room)
    assert ref["has"].sum() > 300
    ctx.close()


IDENTITY_POSE = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def overflow_cloud():
    """(x, y, z, group): group 0 = 200 points of the room; 1 = depths the camera cannot resolve, 0 < zc <= 2^-100 with |xc| or |yc| near 1;
    2 = points whose r6 overflows, zc <= 2^-140 with |xc| or |yc| in [2^31, 2^39]; 3 = xc = yc = 0 with tiny zc."""
    from pointcloudprocessor_amd import synth

    x, y, z, _ = synth.make_cloud(200)
    xs, ys, zs, gs = [x], [y], [z], [np.zeros(200, np.int32)]
    rng = np.random.default_rng(20261020)
    near_one = np.array([1.0, -1.0, 0.75, -0.9375, 1.25, -0.5], np.float32)
    for g, depths, big in ((1, [-100, -101, -113, -126, -127, -140, -149, -120], near_one),
                           (2, [-140, -141, -143, -145, -146, -147, -148, -149], near_one * np.float32(2.0 ** 33))):
        for e in depths:
            for b in big:
                other = np.float32(rng.choice([0.0, 1.0, -0.5, 1e-30])) * (np.float32(1.0) if g == 1 else np.float32(2.0 ** 31))
                for xc, yc in ((b, other), (other, b)):
                    xs.append(np.array([xc], np.float32))
                    ys.append(np.array([yc], np.float32))
                    zs.append(np.array([2.0 ** e], np.float32))
                    gs.append(np.array([g], np.int32))
    for e in (-100, -110, -126, -127, -130, -140, -148, -149, -60, -30, -20, -101, -102, -103, -104, -105):
        xs.append(np.array([0.0 if e % 2 else -0.0], np.float32))
        ys.append(np.array([0.0], np.float32))
        zs.append(np.array([2.0 ** e], np.float32))
        gs.append(np.array([3], np.int32))
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(zs), np.concatenate(gs)


@pytest.mark.parametrize("k3", [0.0, -0.0])
def test_lanes_whose_r6_overflows_are_rejected_like_the_reference_rejects_them(gpu_ctx_factory, oracle, k3):
    from pointcloudprocessor_amd import synth

    cd = camera(dict(k3=k3))
    x, y, z, group = overflow_cloud()
    assert (group == 1).sum() == 96 and (group == 2).sum() == 96 and (group == 3).sum() == 16
    assert (z[group != 0] > 0).all() and (z[group == 1] <= 2.0 ** -100).all() and (z[group == 2] <= 2.0 ** -140).all()
    poses = np.concatenate([np.array([IDENTITY_POSE]), np.asarray(synth.make_trajectory(3)[0], np.float64).reshape(-1, 7)])
    w2c, _ = oracle.pose_to_matrices(poses[0])
    assert np.array_equal(np.asarray(w2c).reshape(3, 4), np.eye(3, 4, dtype=np.float32))
    # r6 as the projection forms it, in fp64: finite for group 1, infinite for group 2
    with np.errstate(all="ignore"):
        xn, yn = x.astype(np.float64) / z.astype(np.float64), y.astype(np.float64) / z.astype(np.float64)
        r2 = xn * xn + yn * yn
        r6 = r2 * (r2 * r2)
    assert np.isfinite(r6[group == 1]).all() and np.isinf(r6[group == 2]).all() and (r6[group == 3] == 0).all()
    images = [synth.make_image(f, 480, 270) for f in range(len(poses))]
    s = dict(x=x, y=y, z=z, poses=poses, images=images)
    # the oracle alone, one keyframe (the identity pose): groups 1 and 2 rejected, group 3 accepted
    ocam, ocp = cam_struct(oracle, cd), oracle.default_cull_params()
    alone = oracle.colorize(ocam, ocp, x, y, z, poses[:1], images[:1], threads=1, want_top=False)
    assert not alone["has"][group == 1].any() and not alone["has"][group == 2].any()
    assert alone["has"][group == 3].all()
    keep, _, _ = oracle.cull_frame(ocam, ocp, w2c, x, y, z)
    assert not keep[(group == 1) | (group == 2)].any() and keep[group == 3].all()
    ctx = loaded_context(gpu_ctx_factory, cd, s)
    assert ctx.selftest_k3_term(samples=0)[1]
    ref = compare_with_oracle(ctx, oracle, cd, s)
    assert ref["has"][group == 3].all()
    ctx.close()
