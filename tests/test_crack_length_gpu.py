"""The crack lengths on the map on the device ("Crack lengths on the map"): pcp_crack_lengths and its fetches against
the library's CPU form and the restatement in _crack_length_ref.py, both fed the device's own fetched views and sums, by exact
equality, on the component cases of the CPU suite seen through the scene harness of test_crack_fuse_gpu.py (64 x 64, three
keyframes); a permuted upload; the state rules of CL9; and that nothing else moves."""
import numpy as np
import pytest

import _crack_fuse_ref as ref
import _crack_length_ref as cl_ref
import _crack_width_ref as cw_ref
from conftest import cam_struct
from test_crack_fuse_gpu import _case_scene, _ctx, _fuse, _setup, CASE_SHAPE

pytestmark = pytest.mark.gpu

RADIUS = 0.005
CASE_NAMES = ["chain_shuffled", "chain_descending", "chains_touch", "chains_apart", "duplicates", "ring", "one_cell", "non_finite",
              "min_views_1", "min_views_3", "single", "no_crack_point", "uniform", "band", "arc"]


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def cases():
    out = ref.component_cases(RADIUS)
    out["band"] = (cl_ref.band(), np.ones(4000, np.uint32), 1)
    out["arc"] = (cl_ref.arc(), np.ones(4000, np.uint32), 1)
    return out


def _case_setup(ctx, xyz, frames=(0, 1, 2)):
    """the case's points and the wall behind them uploaded and fused: (cloud, the fetched state)"""
    cloud, poses, masks = _case_scene(xyz)
    cam = cw_ref.camera(CASE_SHAPE)
    cam.update(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
    _setup(ctx, cam, cloud, poses, masks)
    got, _ = _fuse(ctx, list(frames), 0, 150)
    return cloud, got


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_lengths_on_the_cpu_cases(gpu_ctx_factory, cases, name):
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    assert set(CASE_NAMES) == set(cases)
    xyz, _, min_views = cases[name]
    k = len(xyz)
    cloud, got = _case_setup(ctx, xyz, () if name == "no_crack_point" else (0, 1, 2))
    views, sum_q = got["views"], got["sum_q"]
    finite = np.isfinite(xyz).all(axis=1)
    if name != "no_crack_point":
        assert (views[:k][finite] >= 1).mean() > 0.9, "the scene is wrong: the case's points are not credited"
    out = ctx.crack_lengths(min_views, RADIUS)
    host = capi.crack_lengths_host(cloud, views, min_views, RADIUS, sum_q)
    want = cl_ref.lengths(cloud, views, min_views, RADIUS, sum_q)
    cl_ref.assert_same(host, want, name + ": host form against the restatement")
    cl_ref.assert_same(out, want, name + ": device against the restatement")
    assert out["cracks"] == len(want["ids"]) and out["path_points"] == len(want["path"])
    # the component table the call leaves is the one pcp_crack_components makes for these parameters
    comp = ctx.crack_components(min_views, RADIUS)
    assert np.array_equal(comp["ids"], out["ids"]) and np.array_equal(comp["label"], want["label"])
    assert np.array_equal(out["pos"] == capi.NO_POS, comp["label"] < 0)
    ctx.crack_fuse_end()
    rows, label = out["rows"], want["label"]
    mine = np.flatnonzero(out["ids"] < k)  # the rows of the case's own points (the wall's come after them)
    wall = np.flatnonzero(out["ids"] >= k)
    # the wall's points are far apart: one-point cracks of length 0
    assert (label[k:] >= 0).sum() == len(wall)
    if name != "no_crack_point":
        assert len(wall) > 1000
    assert not rows[wall, 2:4].any() and np.array_equal(rows[wall, 0], out["ids"][wall]) and np.array_equal(rows[wall, 1], out["ids"][wall])
    if name.startswith("chain_"):
        assert len(mine) == 1 and rows[mine[0], 3] == k - 1 == 4099 and comp["stats"][mine[0], 0] == k
        assert sorted(out["path"][:k].tolist()) == list(range(k))
    elif name == "chains_apart":
        assert len(mine) == 2 and rows[mine, 3].tolist() == [39, 39]
    elif name == "chains_touch":
        assert len(mine) == 1 and rows[mine[0], 3] == 79
    elif name in ("band", "arc"):
        assert len(mine) == 1 and rows[mine[0], 3] > 300
        length = rows[mine[0], 2] * cl_ref.UNIT
        assert (1.99 if name == "band" else 1.56) < length < (2.05 if name == "band" else 1.61)
    elif name == "no_crack_point":
        assert out["cracks"] == 0 and out["path_points"] == 0 and (out["pos"] == capi.NO_POS).all() and out["offsets"].tolist() == [0]
    elif name == "uniform":
        assert len(mine) > 10 and (rows[mine, 3] > 5).any()


def test_a_permuted_upload_gives_the_same_lengths_and_paths(gpu_ctx_factory, cases):
    """on chains (trees, where the double sweep is exact whatever the labels are): the same lengths, and the same paths as
    point sets under the permutation"""
    ctx = _ctx(gpu_ctx_factory)
    long = ref.chain(500, RADIUS, np.random.default_rng(20).permutation(500)) + np.array([0.0, 1.0, 0.0], np.float32)
    xyz = np.concatenate([cases["chains_apart"][0], long]).astype(np.float32)
    k = len(xyz)
    _, _ = _case_setup(ctx, xyz)
    first = ctx.crack_lengths(1, RADIUS)
    ctx.crack_fuse_end()
    perm = np.random.default_rng(21).permutation(k)
    inv = np.empty(k, np.int64)
    inv[perm] = np.arange(k)
    _, _ = _case_setup(ctx, xyz[perm])
    second = ctx.crack_lengths(1, RADIUS)
    ctx.crack_fuse_end()

    def own(out):  # the cracks of the case's own points: (length_q, hops, the path's points)
        return [(int(out["rows"][r, 2]), int(out["rows"][r, 3]), out["path"][out["offsets"][r]:out["offsets"][r + 1]])
                for r in np.flatnonzero(out["ids"] < k)]

    a, b = own(first), own(second)
    assert len(a) == len(b) >= 3 and max(h for _, h, _ in a) > 100
    key = lambda c: (c[0], c[1], int(c[2].min()))  # noqa: E731
    a = sorted(a, key=key)
    b = sorted(((q, h, perm[p]) for q, h, p in b), key=key)  # the second run's points under the first run's indices
    for (qa, ha, pa), (qb, hb, pb) in zip(a, b):
        assert (qa, ha) == (qb, hb) and np.array_equal(np.sort(pa), np.sort(pb))
    # pos is measured from a, and which end is a depends on the indices: the same positions, or mirrored
    for (qa, _, pa), (_, _, pb) in zip(a, b):
        pos_a, pos_b = first["pos"][pa].astype(np.int64), second["pos"][inv[pb]].astype(np.int64)
        assert np.array_equal(np.sort(pos_a), np.sort(pos_b)) or np.array_equal(np.sort(pos_a), np.sort(qa - pos_b))


def test_state_rules_and_windows(gpu_ctx_factory, cases):
    capi = _capi()
    C = capi.C

    def code(fn, *a, **kw):
        with pytest.raises(capi.PcpError) as e:
            fn(*a, **kw)
        return e.value.code

    ctx = gpu_ctx_factory()
    L = ctx.lib
    got = C.c_int64(-1)
    assert code(ctx.crack_lengths) == capi.PCP_ERR_STATE  # CL9: no live fusion
    assert L.pcp_crack_lengths_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, None, None, C.byref(got)) == capi.PCP_ERR_STATE
    assert L.pcp_crack_paths_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, C.byref(got)) == capi.PCP_ERR_STATE
    xyz = cases["uniform"][0][:700]
    cloud, poses, masks = _case_scene(xyz)
    cam = cw_ref.camera(CASE_SHAPE)
    cam.update(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
    _setup(ctx, cam, cloud, poses, masks)
    assert code(ctx.crack_lengths) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    none = ctx.crack_lengths(1, RADIUS)  # zero crack points: success, no rows
    assert none["cracks"] == 0 and none["path_points"] == 0 and (none["pos"] == capi.NO_POS).all() and none["offsets"].tolist() == [0]
    for mv, r in ((0, 0.02), (4097, 0.02), (1, 0.004), (1, 1.5)):
        assert code(ctx.crack_lengths, mv, r) == capi.PCP_ERR_INVALID, (mv, r)
    assert L.pcp_crack_lengths(ctx.h, None, None, None, None) == capi.PCP_ERR_INVALID
    ctx.crack_fuse_add(0, 0, 150)
    # an add ends the table's life
    assert L.pcp_crack_lengths_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, None, None, C.byref(got)) == capi.PCP_ERR_STATE
    assert L.pcp_crack_paths_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, C.byref(got)) == capi.PCP_ERR_STATE
    out = ctx.crack_lengths(1, RADIUS)
    c, e = out["cracks"], out["path_points"]
    assert c > 10 and e > c
    # windows of the table and of the paths; every output optional
    for first, rows in ((0, 1), (3, 5), (c - 2, 10), (c, 4), (c + 7, 4), (3, 0), (c, 0)):
        ids = np.full(rows, -7, np.int32)
        tab = np.full((rows, 7), -7, np.int64)
        off = np.full(rows + 1, -7, np.int64)
        assert L.pcp_crack_lengths_fetch(ctx.h, C.c_int64(first), C.c_int64(rows), capi._ptr(ids), capi._ptr(tab), capi._ptr(off), C.byref(got)) == capi.PCP_OK
        g = got.value
        assert g == max(0, min(rows, c - first))
        assert np.array_equal(ids[:g], out["ids"][first:first + g]) and np.array_equal(tab[:g], out["rows"][first:first + g])
        assert np.array_equal(off[:g + 1], out["offsets"][min(first, c):min(first, c) + g + 1])  # (entry 0 even without a row)
        assert (off[g + 1:] == -7).all()
        assert (ids[g:] == -7).all() and (tab[g:] == -7).all()
    assert L.pcp_crack_lengths_fetch(ctx.h, C.c_int64(0), C.c_int64(c), None, None, None, C.byref(got)) == capi.PCP_OK and got.value == c
    for first, n in ((0, 1), (5, 9), (e - 3, 10), (e, 2)):
        idx = np.full(n, -7, np.int32)
        assert L.pcp_crack_paths_fetch(ctx.h, C.c_int64(first), C.c_int64(n), capi._ptr(idx), C.byref(got)) == capi.PCP_OK
        g = got.value
        assert g == max(0, min(n, e - first)) and np.array_equal(idx[:g], out["path"][first:first + g]) and (idx[g:] == -7).all()
    assert L.pcp_crack_lengths_fetch(ctx.h, C.c_int64(-1), C.c_int64(1), None, None, None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_paths_fetch(ctx.h, C.c_int64(0), C.c_int64(-1), None, None) == capi.PCP_ERR_INVALID
    # twice: the same bytes; another radius: its own table
    again = ctx.crack_lengths(1, RADIUS)
    assert all(out[k].tobytes() == again[k].tobytes() for k in cl_ref.KEYS)
    wider = ctx.crack_lengths(1, 0.008)
    assert wider["cracks"] < c
    # the drops
    ctx.crack_fuse_end()
    assert L.pcp_crack_lengths_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, None, None, C.byref(got)) == capi.PCP_ERR_STATE
    assert code(ctx.crack_lengths) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    ctx.crack_fuse_add(0, 0, 150)
    ctx.crack_lengths(1, RADIUS)
    ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
    assert L.pcp_crack_paths_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, C.byref(got)) == capi.PCP_ERR_STATE
    assert code(ctx.crack_lengths) == capi.PCP_ERR_STATE


def test_nothing_else_moves(gpu_ctx_factory, small_scene):
    """the texels, a colour run, pcp_frame_visible and pcp_crack_components' label, table and later results are as without
    pcp_crack_lengths in the cycle"""
    capi = _capi()
    s = small_scene
    ctx = gpu_ctx_factory()
    ctx.set_camera(cam_struct(capi, s["cam"]), capi.default_cull_params())
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.set_frames(s["poses"])
    for f, (im, mk) in enumerate(zip(s["images"], s["masks"])):
        ctx.upload_image(f, im)
        ctx.upload_mask(f, mk)
    before = ctx.colorize()
    packed = ctx.download_result_packed().copy()
    bgr0, mask0 = ctx.download_image(2)
    vis0 = ctx.frame_visible(2)
    cw0 = ctx.crack_width(2, 0, 150, want=("flags", "width"))

    def cycle(with_lengths):
        ctx.crack_fuse_begin()
        for f in (3, 2, 0):
            ctx.crack_fuse_add(f, 0, 150)
        state = ctx.crack_fuse_fetch()
        outs = []
        if with_lengths:
            outs.append(ctx.crack_lengths(1, 0.05))
        comp = ctx.crack_components(1, 0.05)
        if with_lengths:
            outs.append(ctx.crack_lengths(1, 0.03))  # other parameters: its own table; the next components call is its own again
            comp2 = ctx.crack_components(1, 0.05)
            assert all(np.asarray(comp[k]).tobytes() == np.asarray(comp2[k]).tobytes() for k in comp)
        state2 = ctx.crack_fuse_fetch()
        assert all(state[k].tobytes() == state2[k].tobytes() for k in state)
        ctx.crack_fuse_end()
        return state, comp, outs

    state0, comp0, _ = cycle(False)
    state1, comp1, outs = cycle(True)
    assert comp0["components"] >= 1 and outs[0]["cracks"] == comp0["components"] and np.array_equal(outs[0]["ids"], comp0["ids"])
    assert all(state0[k].tobytes() == state1[k].tobytes() for k in state0)
    assert all(np.asarray(comp0[k]).tobytes() == np.asarray(comp1[k]).tobytes() for k in comp0)
    assert np.array_equal(ctx.download_result_packed(), packed)  # the colour result in place
    bgr1, mask1 = ctx.download_image(2)
    assert bgr0.tobytes() == bgr1.tobytes() and mask0.tobytes() == mask1.tobytes()
    vis1 = ctx.frame_visible(2)
    assert all(np.array_equal(vis0[k], vis1[k]) for k in vis0)
    cw1 = ctx.crack_width(2, 0, 150, want=("flags", "width"))
    assert cw0["flags"].tobytes() == cw1["flags"].tobytes() and cw0["width"].tobytes() == cw1["width"].tobytes()
    after = ctx.colorize()
    assert before["rgb"].tobytes() == after["rgb"].tobytes() and before["has"].tobytes() == after["has"].tobytes()
    # and the lengths are the host form's under the fetched state
    cloud = np.stack([s["x"], s["y"], s["z"]], axis=1).astype(np.float32)
    host = capi.crack_lengths_host(cloud, state1["views"], 1, 0.05, state1["sum_q"]) if len(cloud) <= 65536 else None
    if host is not None:
        cl_ref.assert_same(outs[0], host, "small scene")
