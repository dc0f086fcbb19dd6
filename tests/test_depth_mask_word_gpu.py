"""The depth pass refines a tile's mask word from the copy it loaded at the top of the word (it stores
`(word & ~in_range) | seen` without reading the word again).  The tile-mask stage in front of it rewrites every word a pass
touches at tile level, and the pass then clears, among the keyframes of its range, those in which no lane of the tile is a
colouring candidate.  So after passes over ranges that cut the 32-keyframe words anywhere: the bits of the latest range are
those a single pass over every keyframe leaves; no bit that pass leaves set is ever clear (a cleared pair would lose colour
samples); words outside the range are untouched; and the colours are the oracle's."""
import numpy as np
import pytest

from conftest import cam_struct

pytestmark = pytest.mark.gpu

N, F = 3000, 70  # three mask words, the last one ragged; 47 tiles, the last one ragged


def _bits(a, b):
    """(3,) uint32: the mask bits of keyframes [a, b)"""
    f = np.arange(96)
    sel = ((f >= a) & (f < b)).reshape(3, 32)
    return (sel * (np.uint64(1) << np.arange(32, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


@pytest.mark.parametrize("cuts", [(0, 70), (0, 1, 31, 32, 33, 64, 69, 70), (0, 40, 70), (40, 70, 0, 40), (33, 34, 0, 33, 34, 70)])
def test_ranged_depth_passes_refine_their_range_and_lose_no_pair(gpu_ctx_factory, oracle, cuts):
    from pointcloudprocessor_amd import capi, synth

    cd = synth.camera_dict("tiny")
    x, y, z, _ = synth.make_cloud(N)
    poses, _ = synth.make_trajectory(F)
    imgs = [synth.make_image(f % 4, cd["image_width"], cd["image_height"]) for f in range(F)]
    ref = oracle.colorize(cam_struct(oracle, cd), oracle.default_cull_params(), x, y, z, poses, imgs, threads=8, want_top=False)
    assert ref["has"].sum() > 300
    ctx = gpu_ctx_factory()
    ctx.set_camera(cam_struct(capi, cd))
    ctx.upload_cloud(x, y, z)
    ctx.set_frames(poses)
    for f, im in enumerate(imgs):
        ctx.upload_image(f, im)
    ctx.depth_pass()
    whole = ctx.tile_masks()
    assert whole.shape == ((N + 63) // 64, 3) and whole.any() and not (whole[:, 2] >> (F - 64)).any()
    ctx.depth_pass()  # again, over words that are refined already
    assert np.array_equal(ctx.tile_masks(), whole)
    covered = np.zeros(F, bool)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a >= b:
            continue
        before = ctx.tile_masks()
        ctx.depth_pass(a, b)
        covered[a:b] = True
        got, rng = ctx.tile_masks(), _bits(a, b)
        assert np.array_equal(got & rng, whole & rng), (a, b)
        assert not (whole & ~got).any(), (a, b)
        untouched = rng == 0
        assert np.array_equal(got[:, untouched], before[:, untouched]), (a, b)
    assert covered.all()
    got = ctx.colorize_from_depth()
    assert np.array_equal(got["rgb"], ref["rgb"]) and np.array_equal(got["has"], ref["has"])
    ctx.close()
