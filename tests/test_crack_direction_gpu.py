"""The crack directions on the map on the device ("Crack directions on the map"): pcp_crack_directions and its fetch
against the restatement in _crack_direction_ref.py and the library's CPU form, both fed the device's own fetched views --
integers by exact equality, tangents and axes with the bar of test_geometry_gpu.py::test_normals_against_eigh -- on the cases of
the CPU suite seen through the scene harness of test_crack_fuse_gpu.py (64 x 64, three keyframes); a permuted upload; the fetch
windows; the state rules of CD6, one assertion per row of the table in csrc/pcp_crack_map.hpp; and that nothing else moves."""
import numpy as np
import pytest

import _crack_direction_ref as cd_ref
import _crack_fuse_ref as ref
import _crack_length_ref as cl_ref
import _crack_width_ref as cw_ref
from conftest import cam_struct
from test_crack_fuse_gpu import _case_scene, _ctx, _fuse, _setup, CASE_SHAPE

pytestmark = pytest.mark.gpu

RADIUS = 0.005
CASE_NAMES = ["chain_shuffled", "chain_descending", "chains_touch", "chains_apart", "duplicates", "ring", "one_cell", "non_finite",
              "min_views_1", "min_views_3", "single", "no_crack_point", "uniform", "band", "arc", "line", "ypsilon", "helix",
              "two_links", "lonely_pair"]
POINT_KEYS = ("tangent", "anisotropy", "links", "moments")


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def cases():
    out = ref.component_cases(RADIUS)
    out["band"] = (cl_ref.band(), np.ones(4000, np.uint32), 1)
    out["arc"] = (cl_ref.arc(), np.ones(4000, np.uint32), 1)
    out.update(cd_ref.direction_cases())
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
def test_device_directions_on_the_cpu_cases(gpu_ctx_factory, cases, name):
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    assert set(CASE_NAMES) == set(cases)
    xyz, _, min_views = cases[name]
    k = len(xyz)
    cloud, got = _case_setup(ctx, xyz, () if name == "no_crack_point" else (0, 1, 2))
    views = got["views"]
    finite = np.isfinite(xyz).all(axis=1)
    if name != "no_crack_point":
        assert (views[:k][finite] >= 1).mean() > 0.9, "the scene is wrong: the case's points are not credited"
    out = ctx.crack_directions(min_views, RADIUS, want_moments=True)
    want = cd_ref.directions(cloud, views, min_views, RADIUS)
    host = capi.crack_directions_host(cloud, views, min_views, RADIUS)
    cd_ref.assert_integers(host, want, name + ": host form against the restatement")
    cd_ref.assert_integers(out, want, name + ": device against the restatement")
    cd_ref.assert_vectors(out, want, name, "device")
    assert out["cracks"] == len(want["ids"]) and out["crack_points"] == int((want["label"] >= 0).sum())
    assert out["tangent"].dtype == np.float32 and out["anisotropy"].dtype == np.float32
    assert not out["moments"][want["label"] < 0].any() and not out["links"][want["label"] < 0].any()  # CD2: zeros
    # without the moments: the same bytes elsewhere
    lean = ctx.crack_directions(min_views, RADIUS)
    assert "moments" not in lean and all(np.asarray(lean[key]).tobytes() == np.asarray(out[key]).tobytes() for key in lean)
    # the component table the call leaves is the one pcp_crack_components makes for these parameters
    C = capi.C
    rows = out["cracks"]
    ids, stats, box, n_got = np.empty(rows, np.int32), np.empty((rows, 5), np.int64), np.empty((rows, 6), np.float32), C.c_int64()
    assert ctx.lib.pcp_crack_components_fetch(ctx.h, C.c_int64(0), C.c_int64(rows), capi._ptr(ids), capi._ptr(stats), capi._ptr(box),
                                              C.byref(n_got)) == capi.PCP_OK and n_got.value == rows
    comp = ctx.crack_components(min_views, RADIUS)
    assert np.array_equal(comp["ids"], ids) and np.array_equal(comp["stats"], stats) and comp["box"].tobytes() == box.tobytes()
    assert np.array_equal(comp["ids"], out["ids"]) and np.array_equal(comp["label"], want["label"])
    ctx.crack_fuse_end()
    mine = np.flatnonzero(out["ids"] < k)  # the rows of the case's own points (the wall's come after them)
    wall = np.flatnonzero(out["ids"] >= k)
    # the wall's points are far apart: one-point cracks without a link
    assert not out["rows"][wall].any() and not out["axis"][wall].any() and not out["links"][k:].any()
    if name in cd_ref.direction_cases():
        cd_ref.check_known(name, out, k)
    if name.startswith("chain_"):  # a wavefront of one row: the merged branch of the row sums
        assert len(mine) == 1 and out["link_count"][mine[0]] == 2 * (k - 1) == 8198 and out["axis"][mine[0]].tolist() == [1.0, 0.0, 0.0]
    elif name == "chains_apart":  # two cracks in one wavefront: the other branch
        assert len(mine) == 2 and out["link_count"][mine].tolist() == [78.0, 78.0]
    elif name == "chains_touch":
        assert len(mine) == 1 and out["link_count"][mine[0]] == 158
    elif name == "no_crack_point":
        assert out["cracks"] == 0 and out["rows"].shape == (0, 20) and not out["tangent"].any()
    elif name == "uniform":
        assert len(mine) > 10 and (out["link_count"][mine] > 10).any()


def test_a_permuted_upload_gives_the_same_rows(gpu_ctx_factory, cases):
    """CD2: per point the same bytes under the permutation, per crack the same rows (matched by their members)"""
    ctx = _ctx(gpu_ctx_factory)
    xyz = np.concatenate([cases["chains_apart"][0], cases["ypsilon"][0] + np.array([0.0, 0.5, 0.0], np.float32),
                          cases["uniform"][0][:700] + np.array([0.0, 1.0, 0.0], np.float32)]).astype(np.float32)
    k = len(xyz)
    _case_setup(ctx, xyz)
    a = ctx.crack_directions(1, RADIUS, want_moments=True)
    la = ctx.crack_components(1, RADIUS)["label"]
    ctx.crack_fuse_end()
    perm = np.random.default_rng(41).permutation(k)
    _case_setup(ctx, xyz[perm])
    b = ctx.crack_directions(1, RADIUS, want_moments=True)
    ctx.crack_fuse_end()
    assert a["links"][:k].max() >= 2 and a["tangent"][:k].any()
    for key in POINT_KEYS:
        assert a[key][:k][perm].tobytes() == b[key][:k].tobytes(), key
    own_a, own_b = np.flatnonzero(a["ids"] < k), np.flatnonzero(b["ids"] < k)
    assert len(own_a) == len(own_b) > 10
    lowest_b = {}  # a crack of the first run -> its id in the second
    for new, old in enumerate(perm.tolist()):
        if la[old] >= 0:
            lowest_b.setdefault(int(la[old]), new)
    row_b = {int(c): r for r, c in enumerate(b["ids"].tolist())}
    order = [row_b[lowest_b[int(c)]] for c in a["ids"][own_a].tolist()]
    assert sorted(order) == own_b.tolist()
    assert a["rows"][own_a].tobytes() == b["rows"][order].tobytes() and a["axis"][own_a].tobytes() == b["axis"][order].tobytes()


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

    def fetch_code():
        return L.pcp_crack_directions_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, None, C.byref(got))

    def table():
        assert L.pcp_crack_directions_fetch(ctx.h, C.c_int64(0), C.c_int64(2 ** 62), None, None, C.byref(got)) == capi.PCP_OK
        rows = got.value
        ids, tab = np.zeros(rows, np.int32), np.zeros((rows, 20), np.int64)
        assert L.pcp_crack_directions_fetch(ctx.h, C.c_int64(0), C.c_int64(rows), capi._ptr(ids), capi._ptr(tab), C.byref(got)) == capi.PCP_OK
        return ids.tobytes() + tab.tobytes()

    assert code(ctx.crack_directions) == capi.PCP_ERR_STATE and fetch_code() == capi.PCP_ERR_STATE  # no live fusion
    xyz = np.concatenate([cases["ypsilon"][0], cases["uniform"][0][:700] + np.array([0.0, 0.2, 0.0], np.float32)]).astype(np.float32)
    cloud, poses, masks = _case_scene(xyz)
    cam = cw_ref.camera(CASE_SHAPE)
    cam.update(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
    _setup(ctx, cam, cloud, poses, masks)
    assert code(ctx.crack_directions) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    assert fetch_code() == capi.PCP_ERR_STATE  # pcp_crack_fuse_begin: dropped
    none = ctx.crack_directions(1, RADIUS, want_moments=True)  # zero crack points: success, no rows, zeros
    assert none["cracks"] == 0 and none["crack_points"] == 0 and not none["tangent"].any() and not none["moments"].any()
    assert fetch_code() == capi.PCP_OK and got.value == 0
    for mv, r in ((0, 0.02), (4097, 0.02), (1, 0.004), (1, 1.5)):
        with pytest.raises(capi.PcpError) as e:
            ctx.crack_directions(mv, r)
        assert e.value.code == capi.PCP_ERR_INVALID and "pcp_crack_directions:" in str(e.value), (mv, r)
    assert L.pcp_crack_directions(ctx.h, None, None, None, None, None, None, None) == capi.PCP_ERR_INVALID
    assert fetch_code() == capi.PCP_OK  # (a call refused by its parameter checks changes nothing)
    ctx.crack_fuse_add(0, 0, 150)
    assert fetch_code() == capi.PCP_ERR_STATE  # pcp_crack_fuse_add: invalid
    out = ctx.crack_directions(1, RADIUS)
    c = out["cracks"]
    assert c > 10 and fetch_code() == capi.PCP_OK  # pcp_crack_directions: replaced
    mine = table()
    # the windows; every output optional
    for first, rows in ((0, 1), (3, 5), (c - 2, 10), (c, 4), (c + 7, 4), (3, 0), (c, 0)):
        ids = np.full(rows, -7, np.int32)
        tab = np.full((rows, 20), -7, np.int64)
        assert L.pcp_crack_directions_fetch(ctx.h, C.c_int64(first), C.c_int64(rows), capi._ptr(ids), capi._ptr(tab), C.byref(got)) == capi.PCP_OK
        g = got.value
        assert g == max(0, min(rows, c - first))
        assert np.array_equal(ids[:g], out["ids"][first:first + g]) and np.array_equal(tab[:g], out["rows"][first:first + g])
        assert (ids[g:] == -7).all() and (tab[g:] == -7).all()
    assert L.pcp_crack_directions_fetch(ctx.h, C.c_int64(0), C.c_int64(c), None, None, None) == capi.PCP_OK
    assert L.pcp_crack_directions_fetch(ctx.h, C.c_int64(-1), C.c_int64(1), None, None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_directions_fetch(ctx.h, C.c_int64(0), C.c_int64(-1), None, None, None) == capi.PCP_ERR_INVALID
    # pcp_crack_components / _lengths / _skeleton keep them, with other parameters too
    ctx.crack_components(1, 0.008)
    assert table() == mine
    lengths = ctx.crack_lengths(1, RADIUS)
    assert table() == mine
    ctx.crack_skeleton(1, RADIUS, 0.01)
    assert table() == mine
    # a directions call replaces the components, keeps the lengths and the skeleton made before it
    wider = ctx.crack_directions(1, 0.008)
    assert wider["cracks"] < c and table() != mine
    assert L.pcp_crack_components_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, None, None, C.byref(got)) == capi.PCP_OK
    ids, rows7 = np.zeros(c, np.int32), np.zeros((c, 7), np.int64)
    assert L.pcp_crack_lengths_fetch(ctx.h, C.c_int64(0), C.c_int64(c), capi._ptr(ids), capi._ptr(rows7), None, C.byref(got)) == capi.PCP_OK
    assert got.value == c and np.array_equal(ids, lengths["ids"]) and np.array_equal(rows7, lengths["rows"])
    assert L.pcp_crack_skeleton_cracks_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, C.byref(got)) == capi.PCP_OK and got.value == 1
    # twice: the same bytes
    again = ctx.crack_directions(1, RADIUS)
    assert all(np.asarray(out[k]).tobytes() == np.asarray(again[k]).tobytes() for k in out) and table() == mine
    # the drops
    ctx.crack_fuse_end()
    assert fetch_code() == capi.PCP_ERR_STATE and code(ctx.crack_directions) == capi.PCP_ERR_STATE  # pcp_crack_fuse_end

    def live():
        ctx.crack_fuse_begin()
        ctx.crack_fuse_add(0, 0, 150)
        ctx.crack_directions(1, RADIUS)
        assert fetch_code() == capi.PCP_OK

    live()
    ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
    assert fetch_code() == capi.PCP_ERR_STATE  # the cloud uploads
    live()
    ctx.set_frames(np.asarray(poses, np.float64))
    assert fetch_code() == capi.PCP_ERR_STATE  # pcp_set_frames
    for f, m in enumerate(masks):
        ctx.upload_mask(f, m)
    live()
    cull = capi.default_cull_params()
    cull.enable_depth_buffer_culling = 0
    ctx.set_camera(cam_struct(capi, cam), cull)
    assert fetch_code() == capi.PCP_ERR_STATE and code(ctx.crack_directions) == capi.PCP_ERR_STATE  # pcp_set_camera


def test_nothing_else_moves(gpu_ctx_factory, small_scene):
    """the texels, a colour run, pcp_frame_visible, the fused state and pcp_crack_components' label and table are as without
    pcp_crack_directions in the cycle; and the directions are the host form's under the fetched state"""
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

    def cycle(with_directions):
        ctx.crack_fuse_begin()
        for f in (3, 2, 0):
            ctx.crack_fuse_add(f, 0, 150)
        state = ctx.crack_fuse_fetch()
        outs = []
        if with_directions:
            outs.append(ctx.crack_directions(1, 0.05, want_moments=True))
        comp = ctx.crack_components(1, 0.05)
        if with_directions:
            outs.append(ctx.crack_directions(1, 0.03))  # other parameters: its own tables; the next components call is its own again
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
    after = ctx.colorize()
    assert before["rgb"].tobytes() == after["rgb"].tobytes() and before["has"].tobytes() == after["has"].tobytes()
    cloud = np.stack([s["x"], s["y"], s["z"]], axis=1).astype(np.float32)
    if len(cloud) <= 65536:
        host = capi.crack_directions_host(cloud, state1["views"], 1, 0.05)
        for k in ("links", "moments", "ids", "rows"):
            assert np.array_equal(outs[0][k], host[k]), k
        assert np.array_equal(outs[0]["tangent"].any(axis=1), host["tangent"].any(axis=1))
