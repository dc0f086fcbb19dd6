"""The coarse registration on the device ("Coarse registration") against its host twin, bit for bit, on the smallest
shapes at which the kernels can go wrong, and on the room scene; then the state rules of CG7, one assertion each.  No case
provokes a fault: every refusal is a check that returns before any launch."""
import functools

import numpy as np
import pytest

import _coarse_ref as ref
import _register_ref as rref
from conftest import cam_struct

pytestmark = pytest.mark.gpu
F = np.float32


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


_CTX = {}


def _ctx(make):
    """one context for the file; every test uploads the cloud and sets the base it needs"""
    if not _CTX:
        _CTX["ctx"] = make()
    return _CTX["ctx"]


def _upload(ctx, xyz, base=None):
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    if base is not None:
        ctx.compare_set_base(base)


def _same_descriptors(got, host):
    for k in ("desc", "total", "state"):
        assert np.array_equal(got[k], host[k]), k
    assert (got["slots"], got["keypoints"], got["valid"]) == (host["slots"], host["keypoints"], host["valid"])


@functools.lru_cache(maxsize=None)
def _room():
    capi = _capi()
    s = ref.room()
    return s, capi.compare_register_coarse_host(s["xyz"], s["normals"], s["base"], s["base_normals"], **ref.ROOM_KW)


# ---- CG2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("stride", [1, 3])
def test_descriptors_in_a_crowded_cell(gpu_ctx_factory, monkeypatch, form, stride):
    """The table of cell starts dense and sparse (PCP_GRID_SPARSE, read per call), every row and every third a keypoint"""
    monkeypatch.setenv("PCP_GRID_SPARSE", form)
    capi = _capi()
    c = ref.crowded()
    # the grid's own formula puts the crowd into one cell: its walk crosses the 512-record tile, its queries fill eleven work items
    assert ref.crowd_occupancy(c) == ref.CROWD_CELL > 512 and ref.CROWD_CELL // stride > 64
    ctx = _ctx(gpu_ctx_factory)
    for side in (0, 1):  # the same cloud as the map, and as the base
        kw = dict(ref.CROWD_KW, map_stride=stride, base_stride=stride)
        _upload(ctx, c["xyz"], c["xyz"] if side == 1 else None)
        got = ctx.coarse_descriptors(side, normals=c["normals"], **kw)
        host = capi.coarse_descriptors_host(side, c["xyz"], c["normals"], **kw)
        _same_descriptors(got, host)
        key = got["state"] != 0
        assert np.array_equal(got["xyz"][key], c["xyz"][::stride][key])
        assert got["valid"] > 64 and int(got["total"].max()) > 512
        # keypoints on the faces of the box: the corners themselves
        corners = np.flatnonzero(np.isin(c["xyz"], (F(0), F(0.3))).all(axis=1))
        assert corners.tolist() == [234, 331, 366, 420, 493, 613, 631, 838]  # (seed 23; rows 234, 366 and 420 are multiples of 3)
        mine = [int(k) for k in corners if k % stride == 0]
        assert len(mine) == (8 if stride == 1 else 3) and all(got["state"][k // stride] != 0 for k in mine)


def test_descriptors_skip_non_finite_rows_and_invalid_normals(gpu_ctx_factory):
    capi = _capi()
    xyz, nrm = ref.blob(200, 3)
    xyz[5], xyz[77, 1] = np.nan, np.inf
    nrm[9], nrm[10], nrm[11, 0] = 0.0, (2e-4, 0, 0), 1.5
    ctx = _ctx(gpu_ctx_factory)
    _upload(ctx, xyz, xyz)
    for side in (0, 1):
        got = ctx.coarse_descriptors(side, normals=nrm, **ref.BLOB_KW)
        _same_descriptors(got, capi.coarse_descriptors_host(side, xyz, nrm, **ref.BLOB_KW))
        assert got["keypoints"] == 195 and not got["state"][[5, 77, 9, 10, 11]].any() and 20 < int(got["total"].max()) <= 198


# ---- CG3 / CG5 -------------------------------------------------------------------------------------------------------------------
def _staged(ctx, base, base_n, mp, map_n, **kw):
    """descriptors of both sides, then the match: (device match, host match, cb, cm) with every keypoint valid"""
    capi = _capi()
    _upload(ctx, mp, base)
    dm = ctx.coarse_descriptors(capi.CG_MAP, normals=map_n, **kw)
    db = ctx.coarse_descriptors(capi.CG_BASE, normals=base_n, **kw)
    assert dm["valid"] == len(mp) and db["valid"] == len(base)
    _same_descriptors(dm, capi.coarse_descriptors_host(0, mp, map_n, **kw))
    _same_descriptors(db, capi.coarse_descriptors_host(1, base, base_n, **kw))
    got = ctx.coarse_match(**kw)
    host = capi.coarse_match_host(db["desc"], dm["desc"], **kw)
    for k in ("pairs", "base_keys", "map_keys"):
        assert np.array_equal(got[k], host[k]), k
    return got, base[got["pairs"][:, 0]], mp[got["pairs"][:, 1]]


@pytest.mark.parametrize("k_base,k_map,copy", [(1, 65, False), (65, 130, False), (64, 1, False), (130, 65, False), (130, 130, True)])
def test_matching_shapes(gpu_ctx_factory, k_base, k_map, copy):
    """One query, a tile of queries and one more; candidates of one tile and one more, and of two tiles and a rest.  The last
    three rows of the map repeat its first three (equal descriptors); with the base a copy of the map they are L1 = 0 twice
    and the tie goes to the lowest ordinal."""
    ctx = _ctx(gpu_ctx_factory)
    mp, map_n = ref.blob(k_map, 11, duplicates=3 if k_map > 6 else 0)
    base, base_n = (mp.copy(), map_n.copy()) if copy else ref.blob(k_base, 12)
    for mutual in (0, 1):
        got, _, _ = _staged(ctx, base, base_n, mp, map_n, **dict(ref.BLOB_KW, mutual=mutual))
        if mutual == 0:
            assert len(got["pairs"]) == k_base  # (ratio_q8 = 256: every best passes)
        if k_map == 1:
            assert (got["base_keys"][:, 1] == np.uint64(ref.NO_KEY)).all()
        if copy:
            assert [int(v) for v in got["base_keys"][:3, 0]] == [0, 1, 2] and [int(v) for v in got["base_keys"][:3, 1]] == [127, 128, 129]
            assert [int(v) for v in got["base_keys"][-3:, 0]] == [0, 1, 2]


@pytest.mark.parametrize("c", [1, 64, 65])
def test_scoring_shapes(gpu_ctx_factory, c):
    """One frame and 67, the identity among them, over 1, 64 and 65 correspondences"""
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    mp, map_n = ref.blob(c, 13)
    T = ref.planted(angle=0.4, shift=0.5)
    inv = np.linalg.inv(T)
    base = rref.moved(mp, inv)  # a rigid copy: the neighbourhoods, and so the descriptors, agree up to rounding
    base_n = (map_n.astype(np.float64) @ inv[:3, :3].T).astype(F)
    got, cb, cm = _staged(ctx, base, base_n, mp, map_n, **ref.BLOB_KW)
    assert len(cb) == c
    pivot, _ = rref.pivot_of(base)
    rng = np.random.default_rng(c)
    q, t = ref.transform_of(T, pivot)
    Rp = np.array(rref.rotation_of(q)).reshape(3, 3)
    frames = [ref.identity_frame(pivot), np.concatenate([Rp.reshape(9), pivot, t])]  # the identity, then the planted motion
    for _ in range(65):
        R = rref.rodrigues(rng.normal(size=3) * 0.05) @ Rp
        frames.append(np.concatenate([R.reshape(9), pivot, np.asarray(t) + rng.normal(size=3) * 0.03]))
    frames = np.array(frames, np.float64)
    for sel in (frames[:1], frames[1:2], frames):
        dev = ctx.coarse_score(sel, flags=True, **ref.BLOB_KW)
        host = capi.coarse_score_host(sel, cb, cm, flags=True, **ref.BLOB_KW)
        assert dev["flags"].shape == (len(sel), c)  # (sized by the correspondences the Context kept, not by a caller's figure)
        assert np.array_equal(dev["counts"], host["counts"]) and np.array_equal(dev["flags"], host["flags"])
    true_pairs = int((np.linalg.norm(rref.moved(cb, T).astype(np.float64) - cm, axis=1) < 1e-4).sum())
    assert dev["counts"][1] >= true_pairs > 0 and dev["counts"][0] == 0
    assert c == 1 or len(set(dev["counts"].tolist())) > 2  # (the perturbed frames split the pairs differently)


# ---- the whole stage ---------------------------------------------------------------------------------------------------------------
def test_the_whole_stage_equals_the_twin_and_the_chain_reaches_the_planted_pose(gpu_ctx_factory):
    capi = _capi()
    s, host = _room()
    ctx = _ctx(gpu_ctx_factory)
    _upload(ctx, s["xyz"], s["base"])
    got = ctx.compare_register_coarse(normals=s["normals"], base_normals=s["base_normals"], **ref.ROOM_KW)
    assert ref.same_report(got, host) is None, ref.same_report(got, host)
    assert got["status"] == ref.FOUND and got["T"].tobytes() == host["T"].tobytes() and np.array_equal(got["inliers"], host["inliers"])
    assert ctx.compare_base_transform()["T"].tobytes() == got["T"].tobytes()
    # the chain on the device, against the fine registration started from the truth
    truth = capi.compare_register_host(s["xyz"], s["normals"], s["base"], T_in=s["T_true"])
    _upload(ctx, s["xyz"], s["base"])
    chain = ctx.coarse_then_fine(normals=s["normals"], base_normals=s["base_normals"], coarse=ref.ROOM_KW)
    gap = ref.corner_gap(chain["T"], truth["T"], s["base"])
    print("chain: status", chain["status"], "gap", gap)
    assert chain["coarse"]["T"].tobytes() == host["T"].tobytes() and chain["status"] == rref.CONVERGED and gap <= 0.0005


def test_base_normals_estimated_on_the_device_and_fed_back(gpu_ctx_factory):
    capi = _capi()
    s, _ = _room()
    ctx = _ctx(gpu_ctx_factory)
    _upload(ctx, s["xyz"], s["base"])
    kw = dict(ref.ROOM_KW, normal_radius=0.1)
    own = ctx.compare_register_coarse(normals=s["normals"], **kw)
    nrm = ctx.compare_base_normals_fetch()
    assert nrm.shape == s["base"].shape and (np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-3).mean() > 0.99
    # the estimate is the normals stage's: the base uploaded as a map gives the same floats
    ctx.upload_cloud(s["base"][:, 0], s["base"][:, 1], s["base"][:, 2])
    ctx.estimate_normals(0.1)
    assert ctx.normals_fetch()["normal"].tobytes() == nrm.tobytes()
    _upload(ctx, s["xyz"], s["base"])
    fed = ctx.compare_register_coarse(normals=s["normals"], base_normals=nrm, **kw)
    assert ref.same_report(own, fed) is None and own["T"].tobytes() == fed["T"].tobytes() and np.array_equal(own["inliers"], fed["inliers"])
    host = capi.compare_register_coarse_host(s["xyz"], s["normals"], s["base"], nrm, **kw)
    assert ref.same_report(own, host) is None and own["T"].tobytes() == host["T"].tobytes()


# ---- the pipeline layer ------------------------------------------------------------------------------------------------------------
def _same_chain(got, want):
    assert got["status"] == want["status"] and got["T"].tobytes() == want["T"].tobytes()
    assert ref.same_report(got["coarse"], want["coarse"]) is None, ref.same_report(got["coarse"], want["coarse"])
    for stage in ("wide", "fine"):
        assert (got[stage] is None) == (want[stage] is None)
        if want[stage] is not None:
            assert got[stage]["T"].tobytes() == want[stage]["T"].tobytes() and got[stage]["iterations"] == want[stage]["iterations"]


def test_the_pipeline_calls_equal_the_contexts(gpu_ctx_factory):
    """PointCloudColorizer.register_base_coarse and coarse_then_fine against the Context's calls made by hand: the base as (x, y, z),
    the map's normals estimated when none of that radius are live, normal_radius handed on to the base's estimate."""
    import types

    from pointcloudprocessor_amd import pipeline

    s, _ = _room()
    ctx = _ctx(gpu_ctx_factory)
    col = pipeline.PointCloudColorizer(types.SimpleNamespace(ctx=ctx))
    base = s["base"]
    columns = (base[:, 0].copy(), base[:, 1].copy(), base[:, 2].copy())

    def by_hand(radius, call):
        _upload(ctx, s["xyz"])
        if radius is not None:
            ctx.estimate_normals(radius)
        ctx.compare_set_base(base)
        return call()

    # the coarse stage alone: both clouds' normals estimated at 0.12, which is not the parameters' default
    _upload(ctx, s["xyz"])
    got = col.register_base_coarse(columns, normal_radius=0.12, **ref.ROOM_KW)
    assert ctx.normals_radius == 0.12 and ctx.n_base == len(base)
    assert ctx.compare_base_transform()["T"].tobytes() == got["T"].tobytes()
    want = by_hand(0.12, lambda: ctx.compare_register_coarse(normal_radius=0.12, **ref.ROOM_KW))
    assert ref.same_report(got, want) is None, ref.same_report(got, want)
    assert got["T"].tobytes() == want["T"].tobytes() and np.array_equal(got["inliers"], want["inliers"]) and got["keypoints_base"] > 1000
    other = ctx.compare_register_coarse(normal_radius=0.1, **ref.ROOM_KW)  # (the radius shows: the base's normals differ)
    assert ref.same_report(other, want) is not None or other["T"].tobytes() != want["T"].tobytes()
    # the chain: the live estimate is of 0.12, so asking for 0.1 estimates again
    got = col.coarse_then_fine(base, normal_radius=0.1, coarse=ref.ROOM_KW)
    assert ctx.normals_radius == 0.1
    _same_chain(got, by_hand(0.1, lambda: ctx.coarse_then_fine(coarse=dict(ref.ROOM_KW, normal_radius=0.1))))
    # the chain with both clouds' normals given: no estimate is made, and it ends where the Context's does
    _upload(ctx, s["xyz"])
    got = col.coarse_then_fine(columns, normals=s["normals"], base_normals=s["base_normals"], coarse=ref.ROOM_KW)
    assert ctx.normals_radius is None and got["status"] == rref.CONVERGED
    _same_chain(got, by_hand(None, lambda: ctx.coarse_then_fine(normals=s["normals"], base_normals=s["base_normals"], coarse=ref.ROOM_KW)))


# ---- CG7: state --------------------------------------------------------------------------------------------------------------------
def test_state_rules(gpu_ctx_factory):
    capi = _capi()
    s, host = _room()
    ctx = _ctx(gpu_ctx_factory)
    _upload(ctx, s["xyz"], s["base"])
    kw = dict(radius=0.03, half_length=0.05, min_points=5)
    # T is replaced, not composed: from any T the call starts at the ORIGINAL rows and ends at the same bytes
    ctx.compare_set_base_transform(ref.planted(angle=0.3, shift=0.2))
    ctx.compare(normals=s["normals"], **kw)
    got = ctx.compare_register_coarse(normals=s["normals"], base_normals=s["base_normals"], **ref.ROOM_KW)
    assert got["T"].tobytes() == host["T"].tobytes()
    with pytest.raises(capi.PcpError) as e:  # the base moved: the compare result is dropped
        ctx.compare_fetch()
    assert e.value.code == capi.PCP_ERR_STATE and "no result" in str(e.value)
    # status 2 leaves T alone
    less = ctx.compare_register_coarse(normals=s["normals"], base_normals=s["base_normals"], **dict(ref.ROOM_KW, min_inliers=host["winner"] + 1))
    assert less["status"] == ref.TOO_FEW_INLIERS and less["T"].tobytes() == host["T"].tobytes()
    assert ctx.compare_base_transform()["T"].tobytes() == host["T"].tobytes()
    # a new base drops the descriptors of the old one; an upload those of the map
    ctx.compare_set_base(s["base"])
    with pytest.raises(capi.PcpError) as e:
        ctx.coarse_match()
    assert e.value.code == capi.PCP_ERR_STATE and "base" in str(e.value)
    ctx.coarse_descriptors(capi.CG_BASE, normals=s["base_normals"], fetch=False, **ref.ROOM_KW)
    ctx.upload_cloud(s["xyz"][:, 0], s["xyz"][:, 1], s["xyz"][:, 2])
    with pytest.raises(capi.PcpError) as e:
        ctx.coarse_match()
    assert e.value.code == capi.PCP_ERR_STATE and "map" in str(e.value)
    # a new estimate of the map's normals drops the map's descriptors: their axes may have been the old one's
    ctx.estimate_normals(0.1)
    ctx.coarse_descriptors(capi.CG_MAP, fetch=False, **ref.ROOM_KW)
    ctx.coarse_match(**ref.ROOM_KW)  # (both sides are live: it runs)
    ctx.estimate_normals(0.15)
    with pytest.raises(capi.PcpError) as e:
        ctx.coarse_match(**ref.ROOM_KW)
    assert e.value.code == capi.PCP_ERR_STATE and "map" in str(e.value)


def test_refusals_on_the_device(gpu_ctx_factory):
    capi = _capi()
    ctx = gpu_ctx_factory()
    xyz, nrm = ref.blob(100, 5)

    def refused(call, code, word):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)

    refused(lambda: ctx.compare_register_coarse(normals=None), capi.PCP_ERR_STATE, "no cloud")
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    refused(lambda: ctx.compare_register_coarse(normals=nrm), capi.PCP_ERR_STATE, "pcp_compare_set_base")
    refused(ctx.compare_base_normals_fetch, capi.PCP_ERR_STATE, "no estimate")
    ctx.compare_set_base(xyz)
    refused(lambda: ctx.compare_register_coarse(base_normals=nrm), capi.PCP_ERR_STATE, "pcp_estimate_normals")
    refused(lambda: ctx.coarse_match(), capi.PCP_ERR_STATE, "pcp_coarse_descriptors")
    refused(lambda: ctx.coarse_score(np.zeros((1, 15))), capi.PCP_ERR_STATE, "pcp_coarse_match")
    for bad in (dict(support_radius=0.3), dict(support_radius=0.01), dict(normal_radius=2.0), dict(inlier_distance=0.6), dict(min_side=0.0),
                dict(side_tolerance=-1.0), dict(min_angle_deg=61.0), dict(base_stride=0), dict(min_neighbours=0), dict(ratio_q8=-1),
                dict(hypotheses=65537), dict(min_inliers=2), dict(support_radius=float("nan"))):
        refused(lambda: ctx.compare_register_coarse(normals=nrm, base_normals=nrm, **bad), capi.PCP_ERR_INVALID, "pcp_compare_register_coarse")
    big = np.tile(xyz, (2700, 1))  # 270 000 rows at stride 1: more than 2^18 keypoints, refused before any launch
    ctx.compare_set_base(big)
    refused(lambda: ctx.coarse_descriptors(capi.CG_BASE, normals=np.tile(nrm, (2700, 1)), base_stride=1), capi.PCP_ERR_RANGE, "raise the stride")


def test_nothing_else_moves(gpu_ctx_factory, small_scene):
    capi = _capi()
    s = small_scene
    ctx = gpu_ctx_factory()
    ctx.set_camera(cam_struct(capi, s["cam"]), capi.default_cull_params())
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.set_frames(s["poses"])
    for f, (im, mk) in enumerate(zip(s["images"], s["masks"])):
        ctx.upload_image(f, im)
        ctx.upload_mask(f, mk)
    colour = ctx.colorize()
    packed = ctx.download_result_packed()
    ctx.estimate_normals(0.5)
    normals = ctx.normals_fetch()
    xyz = np.stack([s["x"], s["y"], s["z"]], axis=1)
    ctx.compare_set_base(rref.moved(xyz, np.linalg.inv(ref.planted(angle=0.5, shift=1.0))))
    got = ctx.compare_register_coarse(support_radius=0.25, normal_radius=0.5, map_stride=8, base_stride=8, ratio_q8=256, min_neighbours=5)
    assert got["keypoints_map"] > 100 and got["keypoints_base"] > 100
    after = ctx.normals_fetch()
    for k in normals:
        assert after[k].tobytes() == normals[k].tobytes(), k
    assert ctx.download_result_packed().tobytes() == packed.tobytes()
    again = ctx.colorize()
    assert again["rgb"].tobytes() == colour["rgb"].tobytes() and again["has"].tobytes() == colour["has"].tobytes()
