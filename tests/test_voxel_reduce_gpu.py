"""The voxel-grid output on the device ("Voxel-grid output") against the restatement in _voxel_reduce_ref.py applied
to the rows pcp_colour_compact returns.  Every comparison is exact equality.

Scenes.  small_scene (20 000 points, of which 1 450 take a colour) at the sparse leaf 0.05 (1 379 of 1 413 voxels hold one row)
and at the dense leaf 1.0 (81 of 88 voxels hold four rows or more).  A scene of 1 450 coloured rows cannot have 1 000 voxels of
four rows at any leaf, so the crowded case -- at least 1 000 voxels with at least four rows -- is a third scene: the coloured
rows of small_scene twelve times each with a centimetre of jitter, at a leaf of 0.1 (1 699 such voxels by the CPU oracle's
colours).  It is also reduced across uploads, with the default table and with one that starts at 64 slots and grows between
the adds.  The preconditions are asserted below on the rows the device returns."""
import numpy as np
import pytest

import _voxel_reduce_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

SPARSE, DENSE, CROWDED, FINE = 0.05, 1.0, 0.1, 0.001


def _views(ctx, capi, s, masks=False):
    ctx.set_camera(cam_struct(capi, s["cam"]))
    e = np.zeros(0, np.float32)
    ctx.upload_cloud(e, e, e)
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
        if masks:
            ctx.upload_mask(f, s["masks"][f])


def _occupancy(leaf, xyz):
    _, cnt = np.unique(ref.cells(leaf, xyz), axis=0, return_counts=True)
    return cnt


def _reduce(ctx, leaf, want_label=False, initial_slots=0):
    ctx.voxel_reduce_begin(leaf, initial_slots)
    rows = ctx.voxel_reduce_add()
    vox = ctx.voxel_reduce_finish()
    got = ctx.voxel_reduce_fetch(want_label=want_label)
    assert len(got["count"]) == vox
    return got, rows


def _same(got, want, with_label=False):
    bad = ref.same(got, want, with_label)
    assert bad is None, f"{bad} differs"


# small_scene coloured in one shot, its compacted rows and their restatement per leaf: computed once, shared, never modified
_BASE = {}


def _base(gpu_ctx_factory, small_scene):
    if not _BASE:
        from pointcloudprocessor_amd import capi

        s = small_scene
        ctx = gpu_ctx_factory()
        _views(ctx, capi, s, masks=True)
        ctx.upload_cloud(s["x"], s["y"], s["z"])
        ctx.colorize(download=False)
        rows = ctx.colour_compact()
        for v in (rows["index"], rows["xyz"], rows["rgb"]):
            v.setflags(write=False)
        want = {leaf: ref.reduce(leaf, rows["xyz"], rows["rgb"]) for leaf in (SPARSE, DENSE, FINE)}
        _BASE.update(ctx=ctx, rows=rows, want=want)
    return _BASE


def test_one_shot_equals_the_restatement(gpu_ctx_factory, small_scene):
    b = _base(gpu_ctx_factory, small_scene)
    ctx, rows = b["ctx"], b["rows"]
    s = small_scene
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.colorize(download=False)
    sparse, dense = _occupancy(SPARSE, rows["xyz"]), _occupancy(DENSE, rows["xyz"])
    print("sparse leaf: voxels", len(sparse), "of one row", int((sparse == 1).sum()), "| dense leaf: voxels", len(dense),
          "of four rows or more", int((dense >= 4).sum()))
    assert rows["count"] > 1000 and 2 * int((sparse == 1).sum()) > len(sparse), "the sparse leaf leaves most voxels with one row"
    assert 4 * int((dense >= 4).sum()) >= 3 * len(dense) and len(dense) >= 64, "the dense leaf leaves most voxels with four rows or more"
    packed = ctx.download_result_packed().copy()
    for leaf in (SPARSE, DENSE):
        got, added = _reduce(ctx, leaf)
        assert added == rows["count"]
        _same(got, b["want"][leaf])
        st = ctx.voxel_reduce_stats()
        assert st["rows"] == added and st["voxels"] == len(got["count"]) and st["wave_partials"] <= added
        # add changes no other state
        assert np.array_equal(ctx.download_result_packed(), packed)
        after = ctx.colour_compact()
        assert after["count"] == rows["count"] and np.array_equal(after["index"], rows["index"])
        assert after["xyz"].tobytes() == rows["xyz"].tobytes() and after["rgb"].tobytes() == rows["rgb"].tobytes()
    ctx.voxel_reduce_end()


# the crowded scene coloured in one shot: computed once, shared, never modified
_CROWD = {}


def _crowd(gpu_ctx_factory, small_scene):
    if not _CROWD:
        from pointcloudprocessor_amd import capi

        b = _base(gpu_ctx_factory, small_scene)
        rng = np.random.default_rng(41)
        seen = b["rows"]["xyz"]
        pts = (np.repeat(seen, 12, 0) + rng.uniform(-0.01, 0.01, (12 * len(seen), 3))).astype(np.float32)
        scene = dict(x=pts[:, 0].copy(), y=pts[:, 1].copy(), z=pts[:, 2].copy())
        ctx = gpu_ctx_factory()
        _views(ctx, capi, small_scene)
        ctx.upload_cloud(scene["x"], scene["y"], scene["z"])
        ctx.colorize(download=False)
        rows = ctx.colour_compact()
        packed = ctx.download_result_packed().copy()
        for v in (rows["index"], rows["xyz"], rows["rgb"], packed, *scene.values()):
            v.setflags(write=False)
        _CROWD.update(ctx=ctx, scene=scene, rows=rows, packed=packed, want=ref.reduce(CROWDED, rows["xyz"], rows["rgb"]))
    return _CROWD


def test_crowded_scene_a_thousand_voxels_of_four_rows(gpu_ctx_factory, small_scene):
    c = _crowd(gpu_ctx_factory, small_scene)
    ctx, rows = c["ctx"], c["rows"]
    occ = _occupancy(CROWDED, rows["xyz"])
    print("crowded scene: rows", rows["count"], "voxels", len(occ), "of four rows or more", int((occ >= 4).sum()))
    assert int((occ >= 4).sum()) >= 1000, "at least 1 000 voxels with at least 4 rows"
    got, added = _reduce(ctx, CROWDED)
    assert added == rows["count"]
    _same(got, c["want"])
    st = ctx.voxel_reduce_stats()
    print("crowded scene:", st)
    assert st["wave_partials"] < added, "rows of one voxel in neighbouring lanes are merged before the global adds"
    ctx.voxel_reduce_end()


def _coloured_shards(ctx, s, bounds, per_shard):
    """the shards of s coloured one after the other against the depth maps merged over all of them (the whole run's colours)"""
    ctx.depth_accum_reset()
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ctx.upload_cloud(s["x"][lo:hi], s["y"][lo:hi], s["z"][lo:hi])
        ctx.depth_pass()
        ctx.depth_accum_merge()
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ctx.upload_cloud(s["x"][lo:hi], s["y"][lo:hi], s["z"][lo:hi])
        ctx.depth_pass()
        ctx.depth_accum_apply()
        ctx.colorize_from_depth(download=False)
        per_shard(lo, hi)


@pytest.mark.parametrize("leaf", [SPARSE, DENSE])
def test_across_uploads_equals_one_shot(gpu_ctx_factory, small_scene, leaf):
    from pointcloudprocessor_amd import capi

    b = _base(gpu_ctx_factory, small_scene)
    s = small_scene
    ctx = gpu_ctx_factory()
    _views(ctx, capi, s)
    added, words = [], []

    def per_shard(lo, hi):
        words.append(ctx.download_result_packed().copy())
        added.append(ctx.voxel_reduce_add())

    ctx.voxel_reduce_begin(leaf)
    _coloured_shards(ctx, s, [0, 6001, 6002 + 7000, len(s["x"])], per_shard)
    whole = b["ctx"]
    whole.upload_cloud(s["x"], s["y"], s["z"])
    whole.colorize(download=False)
    assert np.array_equal(np.concatenate(words), whole.download_result_packed()), "each shard's colours are the whole run's"
    assert sum(added) == b["rows"]["count"] and all(a > 0 for a in added)
    assert ctx.voxel_reduce_finish() == len(b["want"][leaf]["count"])
    _same(ctx.voxel_reduce_fetch(), b["want"][leaf])
    ctx.voxel_reduce_end()


def test_growth_from_a_table_of_64_slots(gpu_ctx_factory, small_scene):
    b = _base(gpu_ctx_factory, small_scene)
    ctx, s = b["ctx"], small_scene
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.colorize(download=False)
    got, added = _reduce(ctx, SPARSE, initial_slots=64)
    st = ctx.voxel_reduce_stats()
    print("growth:", st)
    _same(got, b["want"][SPARSE])
    assert added == b["rows"]["count"] and st["growths"] >= 3 and st["slots"] >= 2 * st["voxels"]
    default, _ = _reduce(ctx, SPARSE)
    assert ctx.voxel_reduce_stats()["growths"] == 0
    _same(got, default)
    ctx.voxel_reduce_end()


@pytest.mark.parametrize("scene,leaf", [("small", SPARSE), ("small", DENSE), ("crowded", CROWDED)])
def test_table_grows_between_adds_while_it_holds_sums(gpu_ctx_factory, small_scene, scene, leaf):
    """The streamed case in small: a table that starts at 64 slots takes four index shards, the first a fiftieth of the
    cloud, so it is rebuilt at a larger size after sums have been written (k_vr_rehash moves keys AND payloads, plane by
    plane).  At the dense leaf every voxel takes rows from several shards, so the moved sums are added to again.
    Byte-identical to the one-shot result."""
    from pointcloudprocessor_amd import capi

    b = _base(gpu_ctx_factory, small_scene)
    if scene == "small":
        s, want, rows, packed = small_scene, b["want"][leaf], b["rows"], None
    else:
        c = _crowd(gpu_ctx_factory, small_scene)
        s, want, rows, packed = c["scene"], c["want"], c["rows"], c["packed"]
    n = len(s["x"])
    ctx = gpu_ctx_factory()
    _views(ctx, capi, small_scene)
    stats, words = [], []

    def per_shard(lo, hi):
        words.append(ctx.download_result_packed().copy())
        assert ctx.voxel_reduce_add() > 0
        stats.append(ctx.voxel_reduce_stats())

    ctx.voxel_reduce_begin(leaf, 64)
    _coloured_shards(ctx, s, [0, n // 50, n // 4 + 1, n // 2 + 3, n], per_shard)
    print("growth between adds (rows, keys, slots, doublings):", [(st["rows"], st["voxels"], st["slots"], st["growths"]) for st in stats])
    if packed is not None:
        assert np.array_equal(np.concatenate(words), packed), "each shard's colours are the whole run's"
    assert stats[0]["rows"] > 0 and stats[-1]["rows"] == rows["count"]
    assert any(st1["growths"] > st0["growths"] for st0, st1 in zip(stats[:-1], stats[1:])), \
        "an add after the first rebuilds a table that holds sums"
    assert stats[-1]["slots"] >= 2 * stats[-1]["voxels"] and stats[-1]["voxels"] == len(want["count"])
    assert ctx.voxel_reduce_finish() == len(want["count"])
    _same(ctx.voxel_reduce_fetch(), want)
    ctx.voxel_reduce_end()


def test_crowded_scene_across_uploads_default_table(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    c = _crowd(gpu_ctx_factory, small_scene)
    s, n = c["scene"], len(c["scene"]["x"])
    ctx = gpu_ctx_factory()
    _views(ctx, capi, small_scene)
    added = []
    ctx.voxel_reduce_begin(CROWDED)
    _coloured_shards(ctx, s, [0, n // 3, 2 * n // 3 + 1, n], lambda lo, hi: added.append(ctx.voxel_reduce_add()))
    assert sum(added) == c["rows"]["count"] and all(a > 0 for a in added)
    assert ctx.voxel_reduce_finish() == len(c["want"]["count"])
    _same(ctx.voxel_reduce_fetch(), c["want"])
    ctx.voxel_reduce_end()


def test_a_refused_add_after_a_successful_one_changes_nothing(gpu_ctx_factory, small_scene):
    """PCP_ERR_RANGE on an accumulation that holds sums.  The second cloud straddles the end of the 1e-4 lattice (104.8576 m):
    its rows inside place new keys in pass A before the rows outside refuse the call, and the rollback has to take exactly
    those keys out again and keep every sum."""
    from pointcloudprocessor_amd import capi

    b = _base(gpu_ctx_factory, small_scene)
    s = small_scene
    leaf, end = 1e-4, 1048576 * 1e-4
    shift = np.float32(end - float(np.median(b["rows"]["xyz"][:, 0])))  # half of the coloured rows end up on either side
    ctx = gpu_ctx_factory()
    _views(ctx, capi, s)
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.colorize(download=False)
    ctx.voxel_reduce_begin(leaf)
    assert ctx.voxel_reduce_add() == b["rows"]["count"]
    before = ctx.voxel_reduce_stats()
    assert before["voxels"] > 0
    # the accumulator outlives set_frames: the keyframes and the cloud move some 100 m along x together
    moved = np.array(s["poses"], np.float64).copy()
    moved[:, 0] += float(shift)
    ctx.set_frames(moved)
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
    ctx.upload_cloud(s["x"] + shift, s["y"], s["z"])
    ctx.colorize(download=False)
    far = ctx.colour_compact()
    inside = np.abs(far["xyz"]).max(1) < end - 0.01
    outside = np.abs(far["xyz"]).max(1) >= end + 0.01
    print("straddling cloud: coloured rows", far["count"], "inside", int(inside.sum()), "outside", int(outside.sum()))
    assert inside.sum() >= 64 and outside.sum() >= 64, "rows on both sides of the end of the lattice"
    with pytest.raises(capi.PcpError) as e:
        ctx.voxel_reduce_add()
    assert e.value.code == capi.PCP_ERR_RANGE
    assert ctx.voxel_reduce_stats() == before, "a failed add leaves the accumulation as it was"
    # ... and the table still takes rows: the first cloud once more, every voxel now holds its rows twice
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.colorize(download=False)
    assert ctx.voxel_reduce_add() == b["rows"]["count"]
    rows = b["rows"]
    want = ref.reduce(leaf, np.concatenate([rows["xyz"], rows["xyz"]]), np.concatenate([rows["rgb"], rows["rgb"]]))
    assert ctx.voxel_reduce_finish() == len(want["count"]) == before["voxels"]
    _same(ctx.voxel_reduce_fetch(), want)
    ctx.voxel_reduce_end()


def test_wavefront_merge_one_key_and_distinct_keys(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    b = _base(gpu_ctx_factory, small_scene)
    s = small_scene
    # every lane on the same key: the whole cloud scaled into the 1 m voxel of small_scene that holds the most coloured rows
    cells, cnt = np.unique(ref.cells(DENSE, b["rows"]["xyz"]), axis=0, return_counts=True)
    cell = cells[np.argmax(cnt)]
    xyz = np.stack([s["x"], s["y"], s["z"]], 1).astype(np.float64)
    lo, hi = xyz.min(0), xyz.max(0)
    blob = ((xyz - lo) / (hi - lo) * 0.9 + 0.05 + cell).astype(np.float32)
    ctx = gpu_ctx_factory()
    _views(ctx, capi, s)
    ctx.upload_cloud(blob[:, 0].copy(), blob[:, 1].copy(), blob[:, 2].copy())
    ctx.colorize(download=False)
    rows = ctx.colour_compact()
    assert rows["count"] >= 256 and len(_occupancy(DENSE, rows["xyz"])) == 1, "more than a few wavefronts of rows, one voxel"
    got, added = _reduce(ctx, DENSE)
    st = ctx.voxel_reduce_stats()
    print("one key:", st)
    _same(got, ref.reduce(DENSE, rows["xyz"], rows["rgb"]))
    assert added == rows["count"] == int(got["count"][0]) and len(got["count"]) == 1
    assert st["global_adds"] < added and st["global_adds"] == 7 * st["wave_partials"]
    ctx.voxel_reduce_end()
    # every lane on a distinct key: small_scene at 1 mm
    base = b["ctx"]
    base.upload_cloud(s["x"], s["y"], s["z"])
    base.colorize(download=False)
    assert (_occupancy(FINE, b["rows"]["xyz"]) == 1).all()
    got, added = _reduce(base, FINE)
    st = base.voxel_reduce_stats()
    print("distinct keys:", st)
    _same(got, b["want"][FINE])
    assert st["wave_partials"] == added == len(got["count"]) and st["global_adds"] == 7 * added
    base.voxel_reduce_end()


def test_labels_and_the_mixed_add(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    s = small_scene
    ctx = gpu_ctx_factory()
    _views(ctx, capi, s, masks=True)
    ctx.set_label_fusion(True)
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.colorize(download=False)
    rows = ctx.colour_compact(want_label=True)
    assert len(np.unique(rows["label"])) >= 2
    want = ref.reduce(DENSE, rows["xyz"], rows["rgb"], rows["label"])
    ctx.voxel_reduce_begin(DENSE)
    assert ctx.voxel_reduce_add() == rows["count"]
    # a result made without fusion does not mix into a labelled accumulation ...
    ctx.set_label_fusion(False)
    ctx.colorize(download=False)
    with pytest.raises(capi.PcpError) as e:
        ctx.voxel_reduce_add()
    assert e.value.code == capi.PCP_ERR_STATE
    # ... and leaves it as it was
    assert ctx.voxel_reduce_stats()["rows"] == rows["count"]
    ctx.voxel_reduce_finish()
    _same(ctx.voxel_reduce_fetch(want_label=True), want, with_label=True)
    # the other way round: labels are not accumulated, out_label is refused
    ctx.voxel_reduce_begin(DENSE)
    ctx.voxel_reduce_add()
    ctx.set_label_fusion(True)
    ctx.colorize(download=False)
    with pytest.raises(capi.PcpError) as e:
        ctx.voxel_reduce_add()
    assert e.value.code == capi.PCP_ERR_STATE
    ctx.voxel_reduce_finish()
    with pytest.raises(capi.PcpError) as e:
        ctx.voxel_reduce_fetch(want_label=True)
    assert e.value.code == capi.PCP_ERR_STATE
    _same(ctx.voxel_reduce_fetch(), want)
    ctx.set_label_fusion(False)
    ctx.voxel_reduce_end()


def test_after_colour_smooth_local_the_smoothed_colours_enter(gpu_ctx_factory, small_scene):
    b = _base(gpu_ctx_factory, small_scene)
    ctx, s = b["ctx"], small_scene
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.colorize(download=False)
    ctx.colour_smooth_local(0.05)
    rows = ctx.colour_compact()
    assert rows["rgb"].tobytes() != b["rows"]["rgb"].tobytes() or rows["count"] != b["rows"]["count"], "the smoothing changes colours"
    got, added = _reduce(ctx, DENSE)
    assert added == rows["count"]
    _same(got, ref.reduce(DENSE, rows["xyz"], rows["rgb"]))
    assert ref.same(got, b["want"][DENSE]) is not None
    ctx.voxel_reduce_end()


def test_state_rules_refusals_and_fetch_windows(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    b = _base(gpu_ctx_factory, small_scene)
    s = small_scene
    ctx = gpu_ctx_factory()

    def refused(call, code=capi.PCP_ERR_STATE):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == code, e.value

    for call in (ctx.voxel_reduce_add, ctx.voxel_reduce_finish, ctx.voxel_reduce_fetch, ctx.voxel_reduce_stats):  # before begin
        refused(call)
    for leaf in (float("nan"), 0.0, 9e-5, 1.5):
        refused(lambda: ctx.voxel_reduce_begin(leaf), capi.PCP_ERR_INVALID)
    refused(ctx.voxel_reduce_stats)  # a refused begin starts nothing
    ctx.voxel_reduce_begin(SPARSE)
    refused(ctx.voxel_reduce_add)  # no colour result
    refused(ctx.voxel_reduce_fetch)  # before finish
    assert ctx.voxel_reduce_stats()["rows"] == 0
    _views(ctx, capi, s)  # the accumulator outlives set_camera, set_frames and the uploads
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    refused(ctx.voxel_reduce_add)  # the upload ended the colour result
    ctx.colorize(download=False)
    assert ctx.voxel_reduce_add() == b["rows"]["count"]
    # a row out of range: PCP_ERR_RANGE, nothing added
    far = s["x"].copy()
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.colorize(download=False)
    before = ctx.voxel_reduce_stats()
    ctx.voxel_reduce_end()
    refused(ctx.voxel_reduce_stats)
    # (small_scene lies within 7 m of the origin: the refusal is provoked with the smallest leaf, whose lattice ends 104.8576 m
    # from it, on the cloud moved 200 m away together with its keyframes)
    moved = np.array(s["poses"], np.float64).copy()
    moved[:, 0] += 200.0
    ctx.set_frames(moved)
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
    ctx.voxel_reduce_begin(1e-4)
    ctx.upload_cloud(far + np.float32(200.0), s["y"], s["z"])
    ctx.colorize(download=False)
    assert ctx.colour_compact(capacity=0)["count"] > 0
    refused(ctx.voxel_reduce_add, capi.PCP_ERR_RANGE)
    st = ctx.voxel_reduce_stats()
    assert st["rows"] == 0 and st["voxels"] == 0, "a failed add leaves the accumulation as it was"
    assert ctx.voxel_reduce_finish() == 0 and len(ctx.voxel_reduce_fetch()["count"]) == 0
    # the accumulation restarts; add after finish is refused until the next begin; windows tile the result
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.colorize(download=False)
    ctx.voxel_reduce_begin(SPARSE)
    ctx.voxel_reduce_add()
    assert ctx.voxel_reduce_stats()["rows"] == before["rows"]
    vox = ctx.voxel_reduce_finish()
    assert vox == ctx.voxel_reduce_finish() == len(b["want"][SPARSE]["count"])
    refused(ctx.voxel_reduce_add)
    whole = ctx.voxel_reduce_fetch()
    _same(whole, b["want"][SPARSE])
    edges = [0, 1, 64, 65, 1000, vox]
    parts = [ctx.voxel_reduce_fetch(lo, hi - lo) for lo, hi in zip(edges[:-1], edges[1:])]
    for k in ("xyz", "rgb", "count"):
        assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes(), k
    assert len(ctx.voxel_reduce_fetch(vox - 2, 10)["count"]) == 2 and len(ctx.voxel_reduce_fetch(vox, 10)["count"]) == 0
    assert len(ctx.voxel_reduce_fetch(vox + 5, 10)["count"]) == 0
    refused(lambda: ctx.voxel_reduce_fetch(-1, 1), capi.PCP_ERR_INVALID)
    # the result outlives a colour reset and an upload; begin drops it
    ctx.colour_reset()
    ctx.upload_cloud(s["x"][:10], s["y"][:10], s["z"][:10])
    _same(ctx.voxel_reduce_fetch(), whole)
    ctx.voxel_reduce_begin(DENSE)
    refused(ctx.voxel_reduce_fetch)
    ctx.voxel_reduce_end()
    refused(ctx.voxel_reduce_finish)
