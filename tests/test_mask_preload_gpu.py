"""The batched passes load a tile's mask words once -- lane l of the tile's wavefront takes word wbase + l, in chunks of 64 words
-- and walk only the words that keep a keyframe of the range.  The depth pass refines the walked words in their lanes and stores
them once per chunk; the whole-run colour call of the default configuration runs a kernel of its own (k_colour_pass_preload) while
its range spans at most 64 words, the old kernel beyond that.  Checked here at the sizes where that can go wrong: ranges that cut
words, one full tile and a one-point tile, a tile with no set word at all, a second chunk of words (more than 2048 keyframes, where
the colour call also takes the old kernel) against exactly 2048 keyframes (64 words, the new kernel), and the staged calls, which
never take the new kernel.  Colours against the oracle's, masks against ctx.tile_masks() of one pass over every keyframe."""
import numpy as np
import pytest

from conftest import cam_struct

pytestmark = pytest.mark.gpu

N, F = 3000, 70  # 47 tiles, the last one ragged; three mask words, the last one ragged
FAR = 192        # points no keyframe sees, one tight cluster: at least one whole tile of them wherever the tiles' borders fall


def small_camera():
    """64 x 36 images and z-buffer: the optics of "tiny" / 7.5 (2112 images stay under 20 MB)"""
    from pointcloudprocessor_amd import synth

    cd = synth.camera_dict("tiny")
    cd.update(fx=cd["fx"] / 7.5, fy=cd["fy"] / 7.5, cx=32.0, cy=18.0, image_width=64, image_height=36, cull_width=64, cull_height=36)
    return cd


def make_scene(n, frames, cd, far=0):
    from pointcloudprocessor_amd import synth

    x, y, z, _ = synth.make_cloud(n)
    if far:
        # 500 m above the room, within a centimetre of each other: above every keyframe's field of view (the cameras pitch by
        # at most 15 degrees) and too far from the room's points to share a tile with them but at the cluster's two ends
        rng = np.random.default_rng(11)
        x = np.concatenate([x, rng.uniform(-0.005, 0.005, far).astype(x.dtype)])
        y = np.concatenate([y, rng.uniform(-0.005, 0.005, far).astype(y.dtype)])
        z = np.concatenate([z, (500.0 + rng.uniform(-0.005, 0.005, far)).astype(z.dtype)])
    poses, _ = synth.make_trajectory(frames)
    four = [synth.make_image(f, cd["image_width"], cd["image_height"]) for f in range(4)]
    return dict(cam=cd, x=x, y=y, z=z, poses=poses, images=[four[f % 4] for f in range(frames)])


def oracle_colours(oracle, s):
    return oracle.colorize(cam_struct(oracle, s["cam"]), oracle.default_cull_params(), s["x"], s["y"], s["z"], s["poses"],
                           s["images"], threads=8, want_top=False)


def loaded_context(factory, s):
    from pointcloudprocessor_amd import capi

    ctx = factory()
    ctx.set_camera(cam_struct(capi, s["cam"]))
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
    return ctx


def same_colours(got, ref):
    return np.array_equal(got["rgb"], ref["rgb"]) and np.array_equal(got["has"], ref["has"])


@pytest.fixture(scope="module")
def ragged(oracle):
    """the first shape and its oracle colours, computed once"""
    from pointcloudprocessor_amd import synth

    s = make_scene(N, F, synth.camera_dict("tiny"))
    s["ref"] = oracle_colours(oracle, s)
    assert s["ref"]["has"].sum() > 300
    return s


def _bits(a, b, words):
    """(words,) uint32: the mask bits of keyframes [a, b)"""
    f = np.arange(32 * words)
    sel = ((f >= a) & (f < b)).reshape(words, 32)
    return (sel * (np.uint64(1) << np.arange(32, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


@pytest.mark.parametrize("cuts", [(0, 5, 37, 69, 70), (37, 70, 5, 37, 0, 5), (31, 33, 0, 31, 33, 65, 65, 70)])
def test_ranges_that_cut_words(gpu_ctx_factory, ragged, cuts):
    """A pass over [a, b) leaves, on the bits of [a, b), what one pass over every keyframe leaves, and clears no bit that pass
    keeps (the bits of a touched word outside [a, b) are the tile level's again: the mask stage in front of the pass rewrites
    the words it touches); words it does not touch stay; a last pass over everything gives the whole pass's masks again."""
    ctx = loaded_context(gpu_ctx_factory, ragged)
    ctx.depth_pass()
    whole = ctx.tile_masks()
    assert whole.shape == ((N + 63) // 64, 3) and whole.any() and not (whole[:, 2] >> (F - 64)).any()
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a >= b:
            continue
        before = ctx.tile_masks()
        ctx.depth_pass(a, b)
        got, rng = ctx.tile_masks(), _bits(a, b, 3)
        assert np.array_equal(got & rng, whole & rng), (a, b)
        assert not (whole & ~got).any(), (a, b)
        assert np.array_equal(got[:, rng == 0], before[:, rng == 0]), (a, b)
    assert same_colours(ctx.colorize_from_depth(), ragged["ref"])
    ctx.depth_pass()
    assert np.array_equal(ctx.tile_masks(), whole)
    assert same_colours(ctx.colorize_from_depth(), ragged["ref"])
    ctx.close()


@pytest.mark.parametrize("n", [64, 65])
def test_one_tile_and_a_one_point_tile(gpu_ctx_factory, oracle, n):
    from pointcloudprocessor_amd import synth

    s = make_scene(n, 33, synth.camera_dict("tiny"))
    ref = oracle_colours(oracle, s)
    assert ref["has"].sum() >= 8
    ctx = loaded_context(gpu_ctx_factory, s)
    assert same_colours(ctx.colorize(), ref)
    masks = ctx.tile_masks()
    assert masks.shape == ((n + 63) // 64, 2) and masks.any() and not (masks[:, 1] >> 1).any()
    ctx.close()


def test_a_tile_that_no_keyframe_sees(gpu_ctx_factory, oracle):
    from pointcloudprocessor_amd import synth

    s = make_scene(N, F, synth.camera_dict("tiny"), far=FAR)
    ref = oracle_colours(oracle, s)
    assert ref["has"][:N].sum() > 300 and not ref["has"][N:].any()
    ctx = loaded_context(gpu_ctx_factory, s)
    got = ctx.colorize()
    assert same_colours(got, ref) and not got["has"][N:].any() and not got["rgb"][N:].any()
    masks = ctx.tile_masks()
    assert masks.shape == ((N + FAR + 63) // 64, 3)
    empty = ~masks.any(axis=1)
    assert empty.any() and not empty.all()
    # ... and a ranged pass leaves no bit of its range in the empty tiles' words (outside the range the touched words hold
    # the tile level's bits again, which the classifier may keep)
    ctx.depth_pass(3, 67)
    assert not (ctx.tile_masks()[empty] & _bits(3, 67, 3)).any()
    assert same_colours(ctx.colorize_from_depth(), ref)
    ctx.close()


@pytest.mark.parametrize("frames", [2048, 2049, 2112])
def test_64_words_and_more(gpu_ctx_factory, oracle, frames):
    """2048 keyframes: 64 words, one chunk, the new colour kernel; 2049 and 2112: 65 and 66 words, the depth pass's second chunk
    (of one and two lanes) and the old colour kernel."""
    s = make_scene(300, frames, small_camera())
    ref = oracle_colours(oracle, s)
    assert ref["has"].sum() >= 30
    ctx = loaded_context(gpu_ctx_factory, s)
    assert same_colours(ctx.colorize(), ref)
    masks = ctx.tile_masks()
    assert masks.shape == (5, (frames + 31) // 32) and masks[:, :64].any()
    if frames > 2048:
        # the scene has work for the second chunk ...
        assert masks[:, 64:].any()
        # ... and a pass that starts in the first chunk's last word and ends in the second chunk leaves the same bits there
        ctx.depth_pass(2040, frames)
        rng = _bits(2040, frames, masks.shape[1])
        assert np.array_equal(ctx.tile_masks() & rng, masks & rng)
        assert same_colours(ctx.colorize_from_depth(), ref)
    ctx.close()


def test_staged_calls_give_the_whole_run_colours(gpu_ctx_factory, ragged):
    ctx = loaded_context(gpu_ctx_factory, ragged)
    ctx.depth_pass()
    whole = ctx.colorize_from_depth()
    assert same_colours(whole, ragged["ref"])
    ctx.colour_reset()
    ctx.colour_pass(0, 37)
    ctx.colour_pass(37, F)
    assert same_colours(ctx.colour_finalise(), whole)
    ctx.close()
