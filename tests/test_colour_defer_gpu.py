"""The whole-run colour call of the default configuration keeps (score, texel index) pairs while it walks the keyframes and
fetches the texels of the entries that are still listed when the walk is over (k_colour_pass_deferred); PCP_COLOUR_DEFER=0 sends
the same call to the kernel that fetches inside the visit (k_colour_pass_preload).  Every case compares three results array for
array -- the default call, the call under the switch, the oracle -- on scenes built so that the list can go wrong: a ragged last
tile, lists that overflow (evictions) beside lists of exactly 0, 1 and 5 entries, equal scores whose order only the
lower-keyframe-first rule decides, across a 32-keyframe word boundary, and depth maps made in ranged pieces that cut words.
(The library's one-shot colour calls always span every keyframe, [0, n_frames): the kernel's first keyframe is 0 in every call
the C ABI can make, so a range that starts elsewhere is reached for the depth pass only.)"""
import numpy as np
import pytest

from conftest import cam_struct

pytestmark = pytest.mark.gpu

N = 3001  # 47 tiles, the last one of 57 points: dead tail lanes, and 12 workgroups of 256 with a partial one


def scene(frames, spacing, repeat=None):
    """tiny camera, N points, a trajectory with `spacing` metres between keyframes and one image per keyframe, all different;
    repeat = (first, count): keyframes first .. first + count - 1 share the pose of `first` (and keep their own images)"""
    from pointcloudprocessor_amd import synth

    cd = synth.camera_dict("tiny")
    x, y, z, _ = synth.make_cloud(N)
    poses, _ = synth.make_trajectory(frames, spacing=spacing)
    if repeat:
        first, count = repeat
        poses[first:first + count] = poses[first]
    images = [synth.make_image(f, cd["image_width"], cd["image_height"]) for f in range(frames)]
    return dict(cam=cd, x=x, y=y, z=z, poses=poses, images=images)


def with_oracle(oracle, s):
    s["ref"] = oracle.colorize(cam_struct(oracle, s["cam"]), oracle.default_cull_params(), s["x"], s["y"], s["z"], s["poses"],
                               s["images"], threads=8, want_top=True)
    return s


def loaded_context(factory, s):
    from pointcloudprocessor_amd import capi

    ctx = factory()
    ctx.set_camera(cam_struct(capi, s["cam"]))
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
    return ctx


def assert_three_equal(monkeypatch, ctx, ref, call):
    monkeypatch.delenv("PCP_COLOUR_DEFER", raising=False)
    deferred = call()
    monkeypatch.setenv("PCP_COLOUR_DEFER", "0")
    immediate = call()
    monkeypatch.delenv("PCP_COLOUR_DEFER")
    for name, got in (("deferred", deferred), ("immediate", immediate)):
        assert np.array_equal(got["rgb"], ref["rgb"]), name
        assert np.array_equal(got["has"], ref["has"]), name
    assert np.array_equal(deferred["rgb"], immediate["rgb"]) and np.array_equal(deferred["has"], immediate["has"])


@pytest.fixture(scope="module")
def dense(oracle):
    """70 keyframes 8 cm apart: a point that is seen at all is seen by many keyframes in a row"""
    return with_oracle(oracle, scene(70, 0.08))


@pytest.fixture(scope="module")
def tied(oracle):
    """50 keyframes, eight of them (28 .. 35, either side of the word boundary at 32) at one pose under eight different images"""
    return with_oracle(oracle, scene(50, 0.12, repeat=(28, 8)))


def test_evictions_and_short_lists(gpu_ctx_factory, monkeypatch, dense):
    count = dense["ref"]["count"]
    # lists of exactly 0, 1 and 5 entries occur beside lists that overflowed
    for c in (0, 1, 5):
        assert (count == c).sum() >= 3, (c, np.bincount(count)[:8])
    assert (count > 5).sum() >= 300 and (count >= 12).sum() >= 150
    ctx = loaded_context(gpu_ctx_factory, dense)
    assert_three_equal(monkeypatch, ctx, dense["ref"], ctx.colorize)
    ctx.close()


def test_equal_scores_keep_the_lower_keyframe_first(gpu_ctx_factory, monkeypatch, tied):
    ref = tied["ref"]
    score, frame = ref["top_score"], ref["top_frame"]
    rep = (frame >= 28) & (frame < 36)
    # points whose whole list comes from the repeated pose: five equal scores, and the rule alone picks 28 .. 32 out of the eight
    full = rep.all(axis=1)
    assert full.sum() >= 10
    assert (score[full] == score[full][:, :1]).all()
    assert (frame[full] == np.arange(28, 33)).all()
    # ... out of eight different texels: another five would give another colour
    assert (ref["top_rgb"][full] != ref["top_rgb"][full][:, :1]).any(axis=1).all()
    ctx = loaded_context(gpu_ctx_factory, tied)
    assert_three_equal(monkeypatch, ctx, ref, ctx.colorize)
    ctx.close()


def test_depth_maps_made_in_ranges_that_cut_words(gpu_ctx_factory, monkeypatch, dense):
    """depth_pass over [37, 70) and [0, 37), then the one-shot colour call from those maps: 70 keyframes end inside the third word"""
    ctx = loaded_context(gpu_ctx_factory, dense)
    ctx.depth_pass(37, 70)
    ctx.depth_pass(0, 37)
    assert_three_equal(monkeypatch, ctx, dense["ref"], ctx.colorize_from_depth)
    ctx.close()
