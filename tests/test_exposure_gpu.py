"""Exposure gains on the GPU ("Exposure gains"): the pair statistics bit for bit against the numpy restatement
(_exposure_ref.py) on the GPU's own lists and on the oracle's, the gained finalise bit for bit against the restatement, the
state rules of the three entry points, and the equalisation property end to end."""
import numpy as np
import pytest

import _exposure_ref as ex
from conftest import cam_struct
from _exposure_ref import K_EXPOSURE, equalisation_ratio, grey_images

pytestmark = pytest.mark.gpu
F = 6


def _scaled(images, k=K_EXPOSURE):
    return [np.clip(im.astype(np.float32) * np.float32(kf), 0, 255).astype(np.uint8) for im, kf in zip(images, k)]


def _setup(ctx, scene, images, poses=None, masks=None):
    from pointcloudprocessor_amd import capi

    ctx.set_camera(cam_struct(capi, scene["cam"]))
    ctx.upload_cloud(scene["x"], scene["y"], scene["z"])
    ctx.set_frames(scene["poses"] if poses is None else poses)
    for f, im in enumerate(images):
        ctx.upload_image(f, im)
        if masks is not None:
            ctx.upload_mask(f, masks[f])
    return ctx


def _accumulate(ctx, splits=None):
    ctx.colour_reset()
    ctx.depth_pass()
    for f0, f1 in splits or [(0, ctx.n_frames)]:
        ctx.colour_pass(f0, f1)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def scaled_images(small_scene):
    return _scaled(small_scene["images"])


@pytest.fixture(scope="module")
def staged(gpu_ctx_factory, small_scene, scaled_images):
    """one context with the scaled images, its raw lists and statistics (left accumulated; tests that change its state
    restore it)"""
    ctx = _setup(gpu_ctx_factory(), small_scene, scaled_images)
    _accumulate(ctx)
    stats = ctx.view_pair_stats()
    counters = ctx.view_pair_stats_counters()
    raw = ctx.colour_finalise(want_top=True)
    packed = ctx.download_result_packed().copy()
    return dict(ctx=ctx, stats=stats, counters=counters, raw=raw, packed=packed)


def test_statistics_equal_the_restatement_bit_for_bit(staged, oracle, small_scene, scaled_images):
    sc, ctx = small_scene, staged["ctx"]
    raw = staged["raw"]
    want = ex.pair_stats(raw["top_frame"], raw["top_rgb"], F)
    assert want[0].sum() > 1000 and (want[0] > 0).sum() >= 20
    assert _same(staged["stats"], want)
    assert np.array_equal(staged["stats"][0], staged["stats"][0].T) and not np.diag(staged["stats"][0]).any()
    ref = oracle.colorize(cam_struct(oracle, sc["cam"]), oracle.default_cull_params(), sc["x"], sc["y"], sc["z"], sc["poses"], scaled_images)
    assert _same(staged["stats"], ex.pair_stats(ref["top_frame"], ref["top_rgb"], F))
    # the default table holds every key of this scene: nothing went to global memory directly
    c = staged["counters"]
    assert c["direct_adds"] == 0 and c["flush_adds"] > 0 and c["wave_partials"] > 0 and c["table_slots"] == 1024
    # the lists built in two passes give the same matrices
    _accumulate(ctx, [(0, 2), (2, F)])
    assert _same(ctx.view_pair_stats(), want)
    # either output alone
    import ctypes as C

    n_only = np.zeros((F, F), np.uint64)
    ctx._check(ctx.lib.pcp_view_pair_stats(ctx.h, n_only.ctypes.data_as(C.c_void_p), None))
    assert np.array_equal(n_only, want[0])


def test_statistics_with_label_fusion_mask_the_top_byte(gpu_ctx_factory, small_scene, scaled_images, staged):
    ctx = gpu_ctx_factory()
    ctx.set_label_fusion(True)
    masks = [np.full_like(m, 255) if f % 2 else m for f, m in enumerate(small_scene["masks"])]
    _setup(ctx, small_scene, scaled_images, masks=masks)
    _accumulate(ctx)
    assert _same(ctx.view_pair_stats(), staged["stats"])
    ctx.close()


def test_clipped_views_are_left_out(gpu_ctx_factory, small_scene, scaled_images):
    images = [im.copy() for im in scaled_images]
    for f, im in enumerate(images):
        im[:, 40 + 30 * f:140 + 30 * f] = 0
        im[:, 250:330] = 255
    ctx = _setup(gpu_ctx_factory(), small_scene, images)
    _accumulate(ctx)
    got = ctx.view_pair_stats()
    raw = ctx.colour_finalise(want_top=True)
    assert ex.excluded_pairs(raw["top_frame"], raw["top_rgb"]) > 0
    want = ex.pair_stats(raw["top_frame"], raw["top_rgb"], F)
    assert want[0].sum() > 100
    assert _same(got, want)
    ctx.close()


def test_one_cell_receives_every_pair(gpu_ctx_factory, small_scene):
    """20 000 points of a plane in front of two nearly identical poses: every pair lands in the cell (0, 1)."""
    from pointcloudprocessor_amd import capi

    cd = small_scene["cam"]
    pose = np.array(small_scene["poses"][0], np.float64)
    pose2 = pose.copy()
    pose2[0] += 0.001
    _, c2w = capi.pose_to_matrices(pose)
    c2w = c2w.reshape(3, 4).astype(np.float64)
    rng = np.random.default_rng(17)
    n = 20000
    u = rng.uniform(30, cd["image_width"] - 30, n)
    v = rng.uniform(30, cd["image_height"] - 30, n)
    pc = np.stack([(u - cd["cx"]) / cd["fx"] * 2.0, (v - cd["cy"]) / cd["fy"] * 2.0, np.full(n, 2.0), np.ones(n)])
    pw = (c2w @ pc).astype(np.float32)
    scene = dict(cam=cd, x=pw[0].copy(), y=pw[1].copy(), z=pw[2].copy(), poses=np.stack([pose, pose2]))
    h, w = cd["image_height"], cd["image_width"]
    images = [np.full((h, w, 3), 100, np.uint8), np.full((h, w, 3), 140, np.uint8)]
    ctx = _setup(gpu_ctx_factory(), scene, images)
    _accumulate(ctx)
    got_n, got_s = ctx.view_pair_stats()
    raw = ctx.colour_finalise(want_top=True)
    want_n, want_s = ex.pair_stats(raw["top_frame"], raw["top_rgb"], 2)
    assert want_n[0, 1] > 15000
    assert got_n[0, 1] == want_n[0, 1] == got_n[1, 0]
    assert np.array_equal(got_n, want_n) and np.array_equal(got_s, want_s)
    assert got_s[0, 1] == 100 * got_n[0, 1] and got_s[1, 0] == 140 * got_n[0, 1]
    ctx.close()


def test_many_keys_and_a_full_table(gpu_ctx_factory, small_scene, monkeypatch):
    """40 keyframes: more distinct cells than a wavefront has lanes; with the table shrunk to four slots the partials that
    find no slot go to global memory directly, and the matrices are the same."""
    from pointcloudprocessor_amd import synth

    cd = small_scene["cam"]
    poses, _ = synth.make_trajectory(40)
    images = _scaled([synth.make_image(f, cd["image_width"], cd["image_height"]) for f in range(40)],
                     [K_EXPOSURE[f % 6] for f in range(40)])
    ctx = _setup(gpu_ctx_factory(), small_scene, images, poses=poses)
    _accumulate(ctx)
    got = ctx.view_pair_stats()
    assert ctx.view_pair_stats_counters()["direct_adds"] == 0
    raw = ctx.colour_finalise(want_top=True)
    want = ex.pair_stats(raw["top_frame"], raw["top_rgb"], 40)
    assert (want[0] > 0).sum() > 64
    assert _same(got, want)
    for log2, slots in (("2", 4), ("0", 1)):
        monkeypatch.setenv("PCP_EXPOSURE_TABLE_LOG2", log2)
        assert _same(ctx.view_pair_stats(), want)
        c = ctx.view_pair_stats_counters()
        assert c["table_slots"] == slots and c["direct_adds"] > 0 and c["flush_adds"] > 0
    monkeypatch.delenv("PCP_EXPOSURE_TABLE_LOG2")
    assert _same(ctx.view_pair_stats(), want)
    ctx.close()


def test_statistics_need_a_live_accumulation(gpu_ctx_factory, small_scene, scaled_images):
    from pointcloudprocessor_amd import capi

    ctx = _setup(gpu_ctx_factory(), small_scene, scaled_images)
    with pytest.raises(capi.PcpError) as e:
        ctx.view_pair_stats()
    assert e.value.code == capi.PCP_ERR_STATE and "pcp_colour_pass" in str(e.value)
    _accumulate(ctx)
    ctx.view_pair_stats()
    ctx.colour_reset()
    with pytest.raises(capi.PcpError) as e:
        ctx.view_pair_stats()
    assert e.value.code == capi.PCP_ERR_STATE
    ctx.close()


def test_unit_gains_change_nothing(staged):
    ctx, raw = staged["ctx"], staged["raw"]
    _accumulate(ctx)
    ctx.set_frame_gains(np.ones(F))
    try:
        got = ctx.colour_finalise(want_top=True)
        assert np.array_equal(got["rgb"], raw["rgb"]) and np.array_equal(got["has"], raw["has"])
        assert np.array_equal(ctx.download_result_packed(), staged["packed"])
        for key in ("top_rgb", "top_score", "top_frame", "count"):
            assert np.array_equal(got[key], raw[key]), key
    finally:
        ctx.set_frame_gains(None)


def test_gained_finalise_equals_the_restatement(staged):
    from pointcloudprocessor_amd import capi

    ctx, raw = staged["ctx"], staged["raw"]
    g = capi.exposure_gains(*staged["stats"])
    assert np.max(np.abs(g - 1.0)) > 0.05
    _accumulate(ctx)
    try:
        for gains in (g, np.full(F, 16.0), np.array([0.5, 2.0, 1e-3, 16.0, 1.0, 3.3])):
            ctx.set_frame_gains(gains)
            got = ctx.colour_finalise(want_top=True)
            rgb, has = ex.finalise(raw["top_score"], raw["top_rgb"], raw["top_frame"], gains)
            assert np.array_equal(got["rgb"], rgb) and np.array_equal(got["has"], has)
            # the lists stay raw
            for key in ("top_rgb", "top_score", "top_frame", "count"):
                assert np.array_equal(got[key], raw[key]), key
            # ... and everything that reads the result sees the gained colours
            w = ctx.download_result_packed()
            assert np.array_equal(np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], 1).astype(np.uint8), rgb)
            cc = ctx.colour_compact()
            assert np.array_equal(cc["rgb"], rgb[has != 0]) and cc["count"] == int(has.sum())
            if gains[0] == 16.0:  # a bright image under the largest gain clamps
                seen = raw["top_frame"][:, 0] >= 0
                listed = raw["top_frame"] >= 0
                lo = np.where(listed, raw["top_rgb"] & 0xFF, 255).min(axis=1)
                bright = seen & (lo >= 16)
                # every listed channel is 255 then; fl32(fl32(255 s) / s) may fall just below 255 and truncate to 254, as
                # the plain finalise does for a view that is 255 (the restatement above has the exact bits)
                assert bright.sum() > 100 and (got["rgb"][bright, 2] >= 254).all() and (got["rgb"][bright, 2] == 255).any()
                b = (raw["top_rgb"][bright] & 0xFF).astype(np.int64)[listed[bright]]
                assert (ex.gained_channel(b, np.float32(16.0)) == 255).all()
        assert (got["rgb"] != raw["rgb"]).any()
    finally:
        ctx.set_frame_gains(None)


def test_gains_and_the_one_shot_calls(staged, small_scene, scaled_images):
    from pointcloudprocessor_amd import capi

    ctx, raw = staged["ctx"], staged["raw"]
    ctx.set_frame_gains(np.full(F, 1.25))
    for call in (ctx.colorize, ctx.colorize_from_depth):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_STATE and "pcp_colour_finalise" in str(e.value)
    ctx.set_frame_gains(None)
    got = ctx.colorize()
    assert np.array_equal(got["rgb"], raw["rgb"]) and np.array_equal(got["has"], raw["has"])
    # pcp_set_frames clears the gains
    ctx.set_frame_gains(np.full(F, 1.25))
    ctx.set_frames(small_scene["poses"])
    for f, im in enumerate(scaled_images):
        ctx.upload_image(f, im)
    got = ctx.colorize()
    assert np.array_equal(got["rgb"], raw["rgb"])
    _accumulate(ctx)


def test_refused_gains_leave_the_setting(staged):
    from pointcloudprocessor_amd import capi

    ctx, raw = staged["ctx"], staged["raw"]
    g = np.array([1.1, 0.9, 1.2, 0.8, 1.0, 1.3])
    _accumulate(ctx)
    ctx.set_frame_gains(g)
    try:
        for bad in (np.nan, 0.0, -1.0, 17.0, np.inf):
            b = g.copy()
            b[3] = bad
            with pytest.raises(capi.PcpError) as e:
                ctx.set_frame_gains(b)
            assert e.value.code == capi.PCP_ERR_INVALID, bad
        for wrong in (g[:5], np.concatenate([g, [1.0]])):
            with pytest.raises(capi.PcpError) as e:
                ctx.set_frame_gains(wrong)
            assert e.value.code == capi.PCP_ERR_INVALID
        got = ctx.colour_finalise()
        rgb, has = ex.finalise(raw["top_score"], raw["top_rgb"], raw["top_frame"], g)
        assert np.array_equal(got["rgb"], rgb) and np.array_equal(got["has"], has)
    finally:
        ctx.set_frame_gains(None)


def test_grey_keyframes_end_to_end(gpu_ctx_factory, small_scene):
    """The uniform-grey scene of the CPU property, on the GPU's numbers, and the pipeline's option."""
    from pointcloudprocessor_amd import capi, pipeline

    images = grey_images(small_scene["cam"])
    eng = pipeline.HipEngine(0)
    try:
        _setup(eng.ctx, small_scene, images)
        _accumulate(eng.ctx)
        n, s = eng.ctx.view_pair_stats()
        raw = eng.ctx.colour_finalise(want_top=True)
        g = capi.exposure_gains(n, s)
        want = ex.gains(*ex.pair_stats(raw["top_frame"], raw["top_rgb"], F))
        assert np.max(np.abs(g - want) / want) <= 1e-10
        ratio = equalisation_ratio(g)
        print("ratio", ratio, "gains", g)
        assert ratio <= 0.5
        col = pipeline.PointCloudColorizer(eng, balance_exposure=True)
        out = col.run()
        assert np.array_equal(col.gains, g)
        rgb, has = ex.finalise(raw["top_score"], raw["top_rgb"], raw["top_frame"], g)
        assert np.array_equal(out["rgb"], rgb) and np.array_equal(out["has"], has)
        # the option leaves no gains behind: the plain run is the plain run
        plain = pipeline.PointCloudColorizer(eng).run()
        assert np.array_equal(plain["rgb"], raw["rgb"])
        with pytest.raises(ValueError):
            pipeline.PointCloudColorizer(eng, rank=0, world=2, balance_exposure=True)
    finally:
        eng.close()
