"""The crack skeletons on the map on the device ("Crack skeletons on the map"): pcp_crack_skeleton and its fetches
against the library's CPU form and the restatement in _crack_skeleton_ref.py, both fed the device's own fetched views and sums,
by exact equality, on the component cases of the CPU suite and on a junction, a loop and a plus seen through the scene harness of
test_crack_length_gpu.py (64 x 64, three keyframes); the growth of the edge set; a permuted upload; the windows of the three
fetches and the state rules of CS9; and that nothing else moves."""
import numpy as np
import pytest

import _crack_fuse_ref as ref
import _crack_skeleton_ref as cs_ref
import _crack_width_ref as cw_ref
from conftest import cam_struct
from test_crack_fuse_gpu import _case_scene, _ctx, _setup
from test_crack_length_gpu import _case_setup

pytestmark = pytest.mark.gpu

RADIUS = 0.005
STEP = 0.01
CASE_NAMES = ["chain_shuffled", "chain_descending", "chains_touch", "chains_apart", "duplicates", "ring", "one_cell", "non_finite",
              "min_views_1", "min_views_3", "single", "no_crack_point", "uniform", "small_y1", "ring1", "plus1"]


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def cases():
    out = ref.component_cases(RADIUS)
    for name, xyz in (("small_y1", cs_ref.small_y(1)), ("ring1", cs_ref.ring_cloud(1)), ("plus1", cs_ref.plus_cloud(1))):
        out[name] = (xyz, np.ones(len(xyz), np.uint32), 1)
    return out


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_skeleton_on_the_cpu_cases(gpu_ctx_factory, cases, name):
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
    out = ctx.crack_skeleton(min_views, RADIUS, STEP)
    host = capi.crack_skeleton_host(cloud, views, min_views, RADIUS, STEP, sum_q)
    want = cs_ref.skeleton(cloud, views, min_views, RADIUS, STEP, sum_q)
    cs_ref.assert_same(host, want, name + ": host form against the restatement")
    cs_ref.assert_same(out, want, name + ": device against the restatement")
    for key in cs_ref.METRES:
        assert np.array_equal(out[key], want[key]), (name, key)
    # CS1: the two tables the call leaves are those of pcp_crack_components and pcp_crack_lengths for these parameters
    C = capi.C
    rows = np.empty((len(want["cracks"]), 7), np.int64)
    fetched = C.c_int64()
    ctx._check(ctx.lib.pcp_crack_lengths_fetch(ctx.h, C.c_int64(0), C.c_int64(len(rows)), None, capi._ptr(rows), None, C.byref(fetched)))
    lengths = ctx.crack_lengths(min_views, RADIUS)
    assert fetched.value == len(rows) == lengths["cracks"] and np.array_equal(rows, lengths["rows"])
    assert np.array_equal(lengths["pos"], want["pos"])
    ctx.crack_fuse_end()
    cracks, label = out["cracks"], want["label"]
    crack_ids = np.unique(label[label >= 0])
    mine = np.flatnonzero(crack_ids < k)  # the rows of the case's own points (the wall's come after them)
    wall = np.flatnonzero(crack_ids >= k)
    if name != "no_crack_point":
        assert len(wall) > 1000
    assert (cracks[wall] == [1, 0, 0, 0, 0, 0]).all()  # the wall's points are far apart: one-node cracks
    if name.startswith("chain_"):
        assert len(mine) == 1 and cracks[mine[0], 2:].tolist() == [2, 0, 0, 2] and cracks[mine[0], 0] > 1000
    elif name == "small_y1":
        assert len(mine) == 1 and cracks[mine[0], 2:5].tolist() == [3, 1, 0]
    elif name == "ring1":
        assert len(mine) == 1 and cracks[mine[0], 2:5].tolist() == [0, 0, 1] and cracks[mine[0], 0] == cracks[mine[0], 1] > 100
    elif name == "plus1":
        assert len(mine) == 1 and cracks[mine[0], 2:].tolist() == [4, 1, 0, 4]
    elif name == "no_crack_point":
        assert len(out["ids"]) == 0 and len(out["edges"]) == 0 and len(cracks) == 0 and (out["node"] == -1).all()
    elif name == "uniform":
        assert len(mine) > 10 and (cracks[mine, 3] > 0).any()


def test_the_edge_set_grows_from_its_smallest_size(gpu_ctx_factory, cases, monkeypatch):
    """the set starts at 64 slots for several hundred edges: the walk is rerun on doubled sets, and the rows are the same"""
    ctx = _ctx(gpu_ctx_factory)
    _case_setup(ctx, cases["plus1"][0])
    plain = ctx.crack_skeleton(1, RADIUS, STEP)
    monkeypatch.setenv("PCP_SKELETON_SET_LOG2", "6")
    grown = ctx.crack_skeleton(1, RADIUS, STEP)
    monkeypatch.delenv("PCP_SKELETON_SET_LOG2")
    ctx.crack_fuse_end()
    assert len(plain["edges"]) > 64  # more edges than the smallest set has slots
    for key in cs_ref.KEYS:
        assert plain[key].tobytes() == grown[key].tobytes(), key


def _named(out, old_of):
    """the tables under names that do not depend on the upload order: a node is named by the lowest ORIGINAL index among its
    points (old_of: uploaded index -> original index), a crack by the lowest name among its nodes"""
    node, ids, nodes, edges, cracks = out["node"], out["ids"], out["nodes"], out["edges"], out["cracks"]
    who = np.flatnonzero(node >= 0)
    row = np.searchsorted(ids, node[who])
    name = np.full(len(ids), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(name, row, old_of[who])
    crack_name = np.full(len(cracks), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(crack_name, nodes[:, 0], name)
    members = {}
    for r, p in zip(row.tolist(), old_of[who].tolist()):
        members.setdefault(int(name[r]), []).append(p)
    table = {int(name[r]): (int(crack_name[nodes[r, 0]]), tuple(nodes[r, 1:].tolist()), tuple(sorted(members[int(name[r])]))) for r in range(len(ids))}
    edge_set = sorted((int(name[u]), int(name[v]), int(links)) for u, v, links in edges.tolist())
    summary = {int(crack_name[r]): tuple(cracks[r].tolist()) for r in range(len(cracks))}
    return table, edge_set, summary


def test_a_permuted_upload_gives_the_same_diagram(gpu_ctx_factory, cases):
    """A small Y and a chain, uploaded again with the points of each permuted among themselves except the crack's lowest index
    (the start of CL4's first sweep, so that end a and with it every pos stay where they are): the same nodes as point sets,
    the same edges and summaries, and every id the lowest index of its node under the new order."""
    ctx = _ctx(gpu_ctx_factory)
    y = cases["small_y1"][0]
    chain = ref.chain(300, RADIUS, np.random.default_rng(30).permutation(300)) + np.array([0.0, 0.3, 0.0], np.float32)
    xyz = np.concatenate([y, chain]).astype(np.float32)
    k, ky = len(xyz), len(y)
    cloud, _ = _case_setup(ctx, xyz)
    first = ctx.crack_skeleton(1, RADIUS, STEP)
    ctx.crack_fuse_end()
    assert first["node"][0] >= 0 and first["node"][ky] >= 0, "the scene is wrong: a crack's first point is not credited"
    rng = np.random.default_rng(31)
    perm = np.concatenate([[0], 1 + rng.permutation(ky - 1), [ky], ky + 1 + rng.permutation(k - ky - 1)])
    assert sorted(perm.tolist()) == list(range(k)) and (perm != np.arange(k)).mean() > 0.9
    cloud2, _ = _case_setup(ctx, xyz[perm])
    second = ctx.crack_skeleton(1, RADIUS, STEP)
    ctx.crack_fuse_end()
    n = len(cloud)
    assert np.array_equal(cloud2[k:], cloud[k:])  # (the wall behind the points is the same)
    old_of = np.concatenate([perm, np.arange(k, n)])
    a, b = _named(first, np.arange(n)), _named(second, old_of)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    own = [c for name, c in a[2].items() if name < k]
    assert sorted(c[2:5] for c in own) == [(2, 0, 0), (3, 1, 0)]  # the chain and the Y
    # every id is the lowest uploaded index of its node, which is not where it was
    who = np.flatnonzero(second["node"] >= 0)
    lowest = np.full(n, n, np.int64)
    np.minimum.at(lowest, second["node"][who], who)
    assert np.array_equal(lowest[second["ids"]], second["ids"]) and not np.array_equal(first["ids"], second["ids"])


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

    def fetch_codes():
        return (L.pcp_crack_skeleton_nodes_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, None, C.byref(got)),
                L.pcp_crack_skeleton_edges_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, C.byref(got)),
                L.pcp_crack_skeleton_cracks_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, C.byref(got)))

    assert code(ctx.crack_skeleton) == capi.PCP_ERR_STATE  # CS9: no live fusion
    assert fetch_codes() == (capi.PCP_ERR_STATE,) * 3
    xyz = np.concatenate([cases["small_y1"][0], cases["uniform"][0][:700] + np.array([0.0, 0.2, 0.0], np.float32)]).astype(np.float32)
    cloud, poses, masks = _case_scene(xyz)
    cam = cw_ref.camera((64, 64))
    cam.update(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
    _setup(ctx, cam, cloud, poses, masks)
    assert code(ctx.crack_skeleton) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    none = ctx.crack_skeleton(1, RADIUS)  # zero crack points: success, no rows
    assert len(none["ids"]) == 0 and len(none["edges"]) == 0 and len(none["cracks"]) == 0 and (none["node"] == -1).all()
    assert fetch_codes() == (capi.PCP_OK,) * 3 and got.value == 0
    w_max = cs_ref.w_max(RADIUS)
    below = float(np.float32((w_max - 1) * 2.0 ** -20))
    for mv, r, st in ((0, 0.02, 0.04), (4097, 0.02, 0.04), (1, 0.004, 0.04), (1, 1.5, 3.0), (1, RADIUS, below), (1, RADIUS, 16.5), (1, RADIUS, 0.0),
                      (1, RADIUS, float("nan")), (1, 0.02, 0.019)):
        assert code(ctx.crack_skeleton, mv, r, st) == capi.PCP_ERR_INVALID, (mv, r, st)
    assert L.pcp_crack_skeleton(ctx.h, None, C.c_float(0.04), None, None, None) == capi.PCP_ERR_INVALID
    ctx.crack_fuse_add(0, 0, 150)
    assert fetch_codes() == (capi.PCP_ERR_STATE,) * 3  # an add ends the tables' life
    at = float(np.float32(w_max * 2.0 ** -20))
    edge = ctx.crack_skeleton(1, RADIUS, at)  # CS2: step_q = w_max is taken
    out = ctx.crack_skeleton(1, RADIUS, STEP)
    kn, ke, kc = len(out["ids"]), len(out["edges"]), len(out["cracks"])
    assert kn > kc > 10 and ke > 30 and len(edge["ids"]) > kn
    # every output optional: the counts alone
    prm = capi.CrackLinkParams(1, RADIUS)
    a, b = C.c_int64(), C.c_int64()
    assert L.pcp_crack_skeleton(ctx.h, C.byref(prm), C.c_float(STEP), None, C.byref(a), C.byref(b)) == capi.PCP_OK and (a.value, b.value) == (kn, ke)
    assert L.pcp_crack_skeleton(ctx.h, C.byref(prm), C.c_float(STEP), None, None, None) == capi.PCP_OK
    # windows of the three tables
    for first, rows in ((0, 1), (3, 5), (kn - 2, 10), (kn, 4), (kn + 7, 4), (3, 0)):
        ids = np.full(rows, -7, np.int32)
        tab = np.full((rows, 10), -7, np.int64)
        assert L.pcp_crack_skeleton_nodes_fetch(ctx.h, C.c_int64(first), C.c_int64(rows), capi._ptr(ids), capi._ptr(tab), C.byref(got)) == capi.PCP_OK
        g = got.value
        assert g == max(0, min(rows, kn - first))
        assert np.array_equal(ids[:g], out["ids"][first:first + g]) and np.array_equal(tab[:g], out["nodes"][first:first + g])
        assert (ids[g:] == -7).all() and (tab[g:] == -7).all()
    for first, rows in ((0, 1), (5, 9), (ke - 3, 10), (ke, 2), (ke + 5, 2), (2, 0)):
        tab = np.full((rows, 3), -7, np.int64)
        assert L.pcp_crack_skeleton_edges_fetch(ctx.h, C.c_int64(first), C.c_int64(rows), capi._ptr(tab), C.byref(got)) == capi.PCP_OK
        g = got.value
        assert g == max(0, min(rows, ke - first)) and np.array_equal(tab[:g], out["edges"][first:first + g]) and (tab[g:] == -7).all()
    for first, rows in ((0, 1), (4, 6), (kc - 1, 3), (kc, 2), (1, 0)):
        tab = np.full((rows, 6), -7, np.int64)
        assert L.pcp_crack_skeleton_cracks_fetch(ctx.h, C.c_int64(first), C.c_int64(rows), capi._ptr(tab), C.byref(got)) == capi.PCP_OK
        g = got.value
        assert g == max(0, min(rows, kc - first)) and np.array_equal(tab[:g], out["cracks"][first:first + g]) and (tab[g:] == -7).all()
    assert L.pcp_crack_skeleton_nodes_fetch(ctx.h, C.c_int64(-1), C.c_int64(1), None, None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_skeleton_edges_fetch(ctx.h, C.c_int64(0), C.c_int64(-1), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_skeleton_cracks_fetch(ctx.h, C.c_int64(-1), C.c_int64(0), None, None) == capi.PCP_ERR_INVALID
    # twice: the same bytes; a components call leaves the tables, a lengths call replaces CL7's table and ends them
    again = ctx.crack_skeleton(1, RADIUS, STEP)
    assert all(out[key].tobytes() == again[key].tobytes() for key in cs_ref.KEYS)
    ctx.crack_components(1, 0.008)
    assert fetch_codes() == (capi.PCP_OK,) * 3
    ctx.crack_lengths(1, RADIUS)
    assert fetch_codes() == (capi.PCP_ERR_STATE,) * 3
    # the drops
    ctx.crack_skeleton(1, RADIUS, STEP)
    ctx.crack_fuse_end()
    assert fetch_codes() == (capi.PCP_ERR_STATE,) * 3 and code(ctx.crack_skeleton) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    ctx.crack_fuse_add(0, 0, 150)
    ctx.crack_skeleton(1, RADIUS, STEP)
    ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
    assert fetch_codes() == (capi.PCP_ERR_STATE,) * 3 and code(ctx.crack_skeleton) == capi.PCP_ERR_STATE


def test_nothing_else_moves(gpu_ctx_factory, small_scene):
    """the texels, a colour run, pcp_frame_visible, pcp_crack_width, pcp_crack_components' label and table and pcp_crack_lengths'
    pos, table and paths are as without pcp_crack_skeleton in the cycle"""
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

    def cycle(with_skeleton):
        ctx.crack_fuse_begin()
        for f in (3, 2, 0):
            ctx.crack_fuse_add(f, 0, 150)
        state = ctx.crack_fuse_fetch()
        outs = []
        if with_skeleton:
            outs.append(ctx.crack_skeleton(1, 0.05))
        comp = ctx.crack_components(1, 0.05)
        if with_skeleton:
            outs.append(ctx.crack_skeleton(1, 0.03, 0.2))  # other parameters: its own tables
        lengths = ctx.crack_lengths(1, 0.05)
        comp2 = ctx.crack_components(1, 0.05)
        assert all(np.asarray(comp[k]).tobytes() == np.asarray(comp2[k]).tobytes() for k in comp)
        state2 = ctx.crack_fuse_fetch()
        assert all(state[k].tobytes() == state2[k].tobytes() for k in state)
        ctx.crack_fuse_end()
        return state, comp, lengths, outs

    state0, comp0, len0, _ = cycle(False)
    state1, comp1, len1, outs = cycle(True)
    assert comp0["components"] >= 1 and len(outs[0]["cracks"]) == comp0["components"]
    assert all(state0[k].tobytes() == state1[k].tobytes() for k in state0)
    assert all(np.asarray(comp0[k]).tobytes() == np.asarray(comp1[k]).tobytes() for k in comp0)
    assert all(np.asarray(len0[k]).tobytes() == np.asarray(len1[k]).tobytes() for k in len0)
    assert np.array_equal(ctx.download_result_packed(), packed)  # the colour result in place
    bgr1, mask1 = ctx.download_image(2)
    assert bgr0.tobytes() == bgr1.tobytes() and mask0.tobytes() == mask1.tobytes()
    vis1 = ctx.frame_visible(2)
    assert all(np.array_equal(vis0[k], vis1[k]) for k in vis0)
    cw1 = ctx.crack_width(2, 0, 150, want=("flags", "width"))
    assert cw0["flags"].tobytes() == cw1["flags"].tobytes() and cw0["width"].tobytes() == cw1["width"].tobytes()
    after = ctx.colorize()
    assert before["rgb"].tobytes() == after["rgb"].tobytes() and before["has"].tobytes() == after["has"].tobytes()
    # and the skeleton is the host form's under the fetched state, its points those of the components
    cloud = np.stack([s["x"], s["y"], s["z"]], axis=1).astype(np.float32)
    assert np.array_equal(outs[0]["node"] >= 0, comp0["label"] >= 0) and outs[0]["nodes"][:, 2].sum() == comp0["crack_points"]
    if len(cloud) <= 65536:
        host = capi.crack_skeleton_host(cloud, state1["views"], 1, 0.05, None, state1["sum_q"])
        cs_ref.assert_same(outs[0], host, "small scene")
