"""GPU suite of the upload's point order and of the tile bounds with half-extents (csrc/pcp_context.hip spatial_order,
k_up_bounds; csrc/pcp_tile_classify.hpp tile_classify_box): the order is a permutation and a function of the input at sizes
around the tile (64), around 4096 and past two blocks of 4096 (the block of the order refinement that was measured with this
work, profiles/tile_bounds_probe.md: the checks hold for any order) and on degenerate clouds; every point lies inside the sphere
and the box of its tile and of its group; and the masks the box form builds lose no (tile, keyframe) pair that holds a colouring
candidate -- after the depth pass's refinement they are exactly the pairs np_oracle.project_frame finds -- on the room and on
three scenes built to sit where the box differs most from the sphere."""
import numpy as np
import pytest

from conftest import cam_struct

pytestmark = pytest.mark.gpu

F = 16


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi, synth

    c = gpu_ctx_factory()
    c.set_camera(cam_struct(capi, synth.camera_dict("tiny")))
    return c


def check_order_and_bounds(ctx, x, y, z):
    """permutation, the same order from a second upload, containment in fp64 (finite points only)"""
    n = len(x)
    ctx.upload_cloud(x, y, z)
    perm = ctx.cloud_order()
    tiles, groups = ctx.tile_bounds()
    assert perm.shape == (n,) and np.array_equal(np.sort(perm), np.arange(n, dtype=np.int32))
    n_tiles = (n + 63) // 64
    assert tiles.shape == (n_tiles, 8) and groups.shape == ((n_tiles + 15) // 16, 8)
    ctx.upload_cloud(x, y, z)
    assert np.array_equal(ctx.cloud_order(), perm)
    again = ctx.tile_bounds()
    assert np.array_equal(again[0], tiles, equal_nan=True) and np.array_equal(again[1], groups, equal_nan=True)
    p = np.stack([x, y, z], axis=1)[perm].astype(np.float64)
    finite = np.isfinite(p).all(axis=1)
    place = np.arange(n)
    for bounds, span in ((tiles, 64), (groups, 1024)):
        b = bounds.astype(np.float64)[place // span]
        assert (bounds[:, 7] == 0).all()
        d = np.abs(p[finite] - b[finite, 0:3])
        assert (d <= b[finite, 4:7]).all(), span
        assert (np.sqrt((d * d).sum(axis=1)) <= b[finite, 3]).all(), span
    return perm, tiles, groups


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 64 + 1])
def test_sizes_around_the_tile_and_4096(ctx, n):
    from pointcloudprocessor_amd import synth

    x, y, z, _ = synth.make_cloud(n)
    _, tiles, _ = check_order_and_bounds(ctx, x, y, z)
    assert np.isfinite(tiles).all()


def test_copies_of_one_point(ctx):
    n = 5000
    x, y, z = (np.full(n, v, np.float32) for v in (1.25, -0.5, 2.0))
    _, tiles, groups = check_order_and_bounds(ctx, x, y, z)
    # every extent is zero but for the next float up from it
    assert (tiles[:, 3:7] <= 1e-44).all() and (groups[:, 3:7] <= 1e-44).all()


def test_points_on_a_line_along_y(ctx):
    n = 5000
    rng = np.random.default_rng(5)
    y = rng.uniform(-4, 4, n).astype(np.float32)
    x, z = np.full(n, 0.75, np.float32), np.full(n, 1.5, np.float32)
    _, tiles, _ = check_order_and_bounds(ctx, x, y, z)
    assert (tiles[:, 4] <= 1e-44).all() and (tiles[:, 6] <= 1e-44).all() and (tiles[:, 5] > 0).all()


def test_nan_and_infinite_coordinates(ctx):
    from pointcloudprocessor_amd import synth

    x, y, z, _ = (a.copy() for a in synth.make_cloud(5000))
    x[[7, 4100]] = np.nan
    y[[7, 300]] = np.inf
    z[[2500, 4999]] = -np.inf
    z[1234] = np.array([0xFFC00000], np.uint32).view(np.float32)[0]  # a NaN with the sign set
    check_order_and_bounds(ctx, x, y, z)


# ---- the masks against the oracle ----

def room_scene():
    from pointcloudprocessor_amd import synth

    x, y, z, _ = synth.make_cloud(20000)
    return x, y, z


def plane_at_45_degrees():
    """a thin plane x = y: a tile's box is no tighter than its sphere in x and y there, the minimum must pick the sphere"""
    rng = np.random.default_rng(11)
    n = 20000
    s, t = rng.uniform(-3, 3, n), rng.uniform(0.2, 3.5, n)
    e = rng.normal(0, 1e-3, n) / np.sqrt(2)
    return (s + e).astype(np.float32), (s - e).astype(np.float32), t.astype(np.float32)


def wall_through_the_cameras(poses):
    """a wall 0.3 m beside keyframe 8 and along its viewing direction: it crosses z = 0 of that camera and of its neighbours"""
    from oracle import np_oracle

    rng = np.random.default_rng(12)
    n = 20000
    _, c2w = np_oracle.pose_to_matrices(poses[8])
    c2w = np.asarray(c2w, np.float64).reshape(-1, 4)[:3]
    pc = np.stack([np.full(n, 0.3) + rng.normal(0, 1e-3, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-3, 3, n)], axis=1)
    pw = pc @ c2w[:, :3].T + c2w[:, 3]
    return tuple(np.ascontiguousarray(pw[:, a], dtype=np.float32) for a in range(3))


def slab_along_the_border(poses):
    """a slab 2 m in front of keyframe 5 that images along the lower border and across the lower right corner (the image's
    half-extents are 0.425 x 0.239 in normalised coordinates)"""
    from oracle import np_oracle

    rng = np.random.default_rng(13)
    n = 20000
    _, c2w = np_oracle.pose_to_matrices(poses[5])
    c2w = np.asarray(c2w, np.float64).reshape(-1, 4)[:3]
    zc = rng.uniform(2.0, 2.1, n)
    pc = np.stack([zc * rng.uniform(-0.1, 0.6, n), zc * rng.uniform(0.2, 0.28, n), zc], axis=1)
    pw = pc @ c2w[:, :3].T + c2w[:, 3]
    return tuple(np.ascontiguousarray(pw[:, a], dtype=np.float32) for a in range(3))


@pytest.fixture(scope="module")
def keyframes():
    from pointcloudprocessor_amd import synth

    poses, _ = synth.make_trajectory(F)
    four = [synth.make_image(f, 480, 270) for f in range(4)]
    return poses, [four[f % 4] for f in range(F)]


def check_masks_against_oracle(ctx, cloud, poses):
    from oracle import np_oracle
    from pointcloudprocessor_amd import synth

    cd = synth.camera_dict("tiny")
    x, y, z = cloud
    n = len(x)
    ctx.upload_cloud(x, y, z)
    ctx.set_frames(poses)
    perm = ctx.cloud_order()
    ctx.depth_pass()
    masks = ctx.tile_masks()
    n_tiles = (n + 63) // 64
    assert masks.shape == (n_tiles, 1)
    got = ((masks[:, 0:1] >> np.arange(F, dtype=np.uint32)[None, :]) & 1).astype(bool)
    tile_of_point = np.empty(n, np.int64)
    tile_of_point[perm] = np.arange(n) // 64
    want = np.zeros((n_tiles, F), bool)
    for f, pose in enumerate(poses):
        w2c, _ = np_oracle.pose_to_matrices(pose)
        p = np_oracle.project_frame(cd, w2c, x, y, z)
        want[tile_of_point[(p["cell"] >= 0) & (p["pixel"] >= 0)], f] = True
    print("pairs with a candidate", int(want.sum()), "of", want.size, "missing", int((want & ~got).sum()), "extra", int((got & ~want).sum()))
    assert not (want & ~got).any()  # soundness: no pair that holds a candidate was rejected
    assert np.array_equal(got, want)
    return int(want.sum())


def test_masks_of_the_room_against_the_oracle(ctx, keyframes):
    assert check_masks_against_oracle(ctx, room_scene(), keyframes[0]) > 100


@pytest.mark.parametrize("scene", ["plane", "wall", "slab"])
def test_adversarial_scenes_masks_and_colours(ctx, oracle, keyframes, scene):
    from pointcloudprocessor_amd import synth

    poses, images = keyframes
    cloud = {"plane": plane_at_45_degrees, "wall": lambda: wall_through_the_cameras(poses), "slab": lambda: slab_along_the_border(poses)}[scene]()
    assert check_masks_against_oracle(ctx, cloud, poses) > 100
    for f, im in enumerate(images):
        ctx.upload_image(f, im)
    cd = synth.camera_dict("tiny")
    ref = oracle.colorize(cam_struct(oracle, cd), oracle.default_cull_params(), *cloud, poses, images, threads=8, want_top=False)
    got = ctx.colorize()
    print("coloured", int(ref["has"].sum()), "colours differing", int((got["rgb"] != ref["rgb"]).any(axis=1).sum()))
    assert ref["has"].sum() > 100
    assert np.array_equal(got["rgb"], ref["rgb"]) and np.array_equal(got["has"], ref["has"])
