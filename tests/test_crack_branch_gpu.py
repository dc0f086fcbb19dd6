"""The crack branches on the map on the device ("Crack branches on the map"): pcp_crack_branches and its fetches
against the library's CPU form and the restatement in _crack_branch_ref.py, both fed the device's own fetched views and sums, by
exact equality, on the component cases of the CPU suite and on a junction, a loop, a plus and a stem with a twig seen through the
scene harness of test_crack_length_gpu.py (64 x 64, three keyframes), with and without pruning; the tables the call leaves
against those of pcp_crack_skeleton; a permuted upload; the windows of the three fetches and the state rules of CB9; and that
nothing else moves."""
import numpy as np
import pytest

import _crack_branch_ref as cb_ref
import _crack_fuse_ref as ref
import _crack_skeleton_ref as cs_ref
import _crack_width_ref as cw_ref
from conftest import cam_struct
from test_crack_fuse_gpu import _case_scene, _ctx, _setup
from test_crack_length_gpu import _case_setup

pytestmark = pytest.mark.gpu

RADIUS = 0.005
STEP = 0.01
PRUNES = (0.0, 0.05)
CASE_NAMES = ["chain_shuffled", "chain_descending", "chains_touch", "chains_apart", "duplicates", "ring", "one_cell", "non_finite",
              "min_views_1", "min_views_3", "single", "no_crack_point", "uniform", "small_y1", "ring1", "plus1", "twig"]


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def cases():
    out = ref.component_cases(RADIUS)
    for name, xyz in (("small_y1", cs_ref.small_y(1)), ("ring1", cs_ref.ring_cloud(1)), ("plus1", cs_ref.plus_cloud(1)), ("twig", cb_ref.twig())):
        out[name] = (xyz, np.ones(len(xyz), np.uint32), 1)
    return out


def _left_tables(ctx):
    """the component, length and skeleton tables as the fetches serve them now"""
    capi = _capi()
    C, L, ptr = capi.C, ctx.lib, capi._ptr
    got = C.c_int64()
    big = C.c_int64(2 ** 62)
    ctx._check(L.pcp_crack_components_fetch(ctx.h, C.c_int64(0), big, None, None, None, C.byref(got)))
    c = got.value
    cc_ids, cc_stats, cc_box = np.empty(c, np.int32), np.empty((c, 5), np.int64), np.empty((c, 6), np.float32)
    ctx._check(L.pcp_crack_components_fetch(ctx.h, C.c_int64(0), C.c_int64(c), ptr(cc_ids), ptr(cc_stats), ptr(cc_box), C.byref(got)))
    cl_ids, cl_rows, cl_off = np.empty(c, np.int32), np.empty((c, 7), np.int64), np.zeros(c + 1, np.int64)
    ctx._check(L.pcp_crack_lengths_fetch(ctx.h, C.c_int64(0), C.c_int64(c), ptr(cl_ids), ptr(cl_rows), ptr(cl_off), C.byref(got)))
    assert got.value == c
    path = np.empty(int(cl_off[-1]), np.int32)
    ctx._check(L.pcp_crack_paths_fetch(ctx.h, C.c_int64(0), C.c_int64(len(path)), ptr(path), C.byref(got)))
    ctx._check(L.pcp_crack_skeleton_nodes_fetch(ctx.h, C.c_int64(0), big, None, None, C.byref(got)))
    kn = got.value
    ids, nodes = np.empty(kn, np.int32), np.empty((kn, 10), np.int64)
    ctx._check(L.pcp_crack_skeleton_nodes_fetch(ctx.h, C.c_int64(0), C.c_int64(kn), ptr(ids), ptr(nodes), C.byref(got)))
    ctx._check(L.pcp_crack_skeleton_edges_fetch(ctx.h, C.c_int64(0), big, None, C.byref(got)))
    edges = np.empty((got.value, 3), np.int64)
    ctx._check(L.pcp_crack_skeleton_edges_fetch(ctx.h, C.c_int64(0), C.c_int64(len(edges)), ptr(edges), C.byref(got)))
    cracks = np.empty((c, 6), np.int64)
    ctx._check(L.pcp_crack_skeleton_cracks_fetch(ctx.h, C.c_int64(0), C.c_int64(c), ptr(cracks), C.byref(got)))
    assert got.value == c
    return dict(cc_ids=cc_ids, cc_stats=cc_stats, cc_box=cc_box, cl_ids=cl_ids, cl_rows=cl_rows, cl_off=cl_off, path=path, ids=ids, nodes=nodes,
                edges=edges, cracks=cracks)


@pytest.mark.parametrize("prune", PRUNES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_branches_on_the_cpu_cases(gpu_ctx_factory, cases, name, prune):
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
    out = ctx.crack_branches(min_views, RADIUS, STEP, prune)
    left = _left_tables(ctx)
    host = capi.crack_branches_host(cloud, views, min_views, RADIUS, STEP, prune, sum_q)
    want = cb_ref.branches(cloud, views, min_views, RADIUS, STEP, prune, sum_q)
    cb_ref.check_rules(want, prune, name)
    cb_ref.assert_same(host, want, name + ": host form against the restatement")
    cb_ref.assert_same(out, want, name + ": device against the restatement")
    assert out["pruned_branches"] == want["cracks"][:, 4].sum()
    for key in ("axis", "anisotropy", "link_count"):
        assert np.array_equal(out[key], host[key]), (name, key)
    # CB1: the tables the call leaves are those of pcp_crack_skeleton for these parameters (which leaves the branches invalid)
    sk = ctx.crack_skeleton(min_views, RADIUS, STEP)
    after = _left_tables(ctx)
    for key in left:
        assert left[key].tobytes() == after[key].tobytes(), (name, key)
    cs_ref.assert_same(sk, want["skeleton"], name + ": the skeleton")
    assert ctx.lib.pcp_crack_branches_fetch(ctx.h, capi.C.c_int64(0), capi.C.c_int64(1), None, None, None, None) == capi.PCP_ERR_STATE
    ctx.crack_fuse_end()
    # the known answers, and that the cases exercise what they are there for
    branch, rows = want["branch"], want["rows"]
    mine = np.flatnonzero(want["ids"] < k)  # the rows of the case's own points (the wall's come after them)
    wall = np.flatnonzero(want["ids"] >= k)
    if name != "no_crack_point":
        assert len(wall) > 1000 and (rows[wall, 1:7] == [1, 0, 0, -1, -1, 1]).all()  # the wall's points are far apart: one-point branches
    if name.startswith("chain_"):
        assert len(mine) == 1 and rows[mine[0], 3] == 0 and rows[mine[0], 1] > 100 and rows[mine[0], 6] > 1000
    elif name == "chains_apart":
        assert len(mine) == 2 and not rows[mine, 3].any()  # two branches side by side in the cell order: wavefronts that share a row and that do not
    elif name in ("small_y1", "plus1"):
        arms = 3 if name == "small_y1" else 4
        assert len(mine) == arms and (rows[mine, 3] == 1).all() and (branch[:k] == cb_ref.JUNCTION).any()
    elif name == "ring1":
        assert len(mine) == 1 and rows[mine[0], 3] == 0 and rows[mine[0], 2] == rows[mine[0], 1] > 100
    elif name == "twig":
        assert len(mine) == (3 if prune == 0 else 1)
        assert (branch[:k] == cb_ref.PRUNED).any() == (prune > 0) and (branch[:k] == cb_ref.JUNCTION).any() == (prune == 0)
    elif name == "no_crack_point":
        assert len(out["ids"]) == 0 and len(out["edge_branch"]) == 0 and len(out["cracks"]) == 0 and (out["branch"] == -1).all()
    elif name == "uniform":
        assert len(mine) > 10 and (branch[:k] == cb_ref.JUNCTION).any()
        print("uniform: bridges", int((want["edge_branch"] == cb_ref.BRIDGE).sum()), "pruned points", int((branch == cb_ref.PRUNED).sum()),
              "branches with two attachments", int((rows[:, 3] == 2).sum()))
        assert (rows[mine, 3] == 2).any(), "a branch between two junctions"
        if prune > 0:
            assert (branch[:k] == cb_ref.PRUNED).any()
        else:
            assert (want["edge_branch"] == cb_ref.BRIDGE).any(), "component_cases yields a bridge (61 of them with every point credited)"


def _named(out, sk, old_of):
    """the tables under names that do not depend on the upload order: a branch and a node are named by the lowest ORIGINAL index
    among their points (old_of: uploaded index -> original index), a crack by the lowest name among its nodes"""
    branch, ids, rows = out["branch"], out["ids"], out["rows"]
    node, node_ids, nodes = sk["node"], sk["ids"], sk["nodes"]
    big = np.iinfo(np.int64).max
    who = np.flatnonzero(node >= 0)
    node_name = np.full(len(node_ids), big, np.int64)
    np.minimum.at(node_name, np.searchsorted(node_ids, node[who]), old_of[who])
    crack_name = np.full(len(out["cracks"]), big, np.int64)
    np.minimum.at(crack_name, nodes[:, 0], node_name)
    inb = np.flatnonzero(branch >= 0)
    row = np.searchsorted(ids, branch[inb])
    name = np.full(len(ids), big, np.int64)
    np.minimum.at(name, row, old_of[inb])
    members = {}
    for r, p in zip(row.tolist(), old_of[inb].tolist()):
        members.setdefault(r, []).append(p)
    table = {}
    for r in range(len(ids)):
        junctions = tuple(sorted(int(node_name[j]) for j in rows[r, 4:6].tolist() if j >= 0))
        table[int(name[r])] = (int(crack_name[rows[r, 0]]), tuple(rows[r, 1:4].tolist()), junctions, tuple(rows[r, 6:].tolist()),
                               tuple(out["moments"][r].tolist()), tuple(sorted(members[r])))
    outside = {int(old_of[i]): int(branch[i]) for i in np.flatnonzero((branch < 0) & (node >= 0)).tolist()}
    edge_set = sorted((int(node_name[u]), int(node_name[v]), int(name[b]) if b >= 0 else int(b))
                      for (u, v, _), b in zip(sk["edges"].tolist(), out["edge_branch"].tolist()))
    summary = {int(crack_name[r]): tuple(out["cracks"][r].tolist()) for r in range(len(crack_name))}
    metres = {int(name[r]): float(out["length_m"][r]) for r in range(len(ids))}  # CB8: sums in edge-row order, and the rows move
    return table, outside, edge_set, summary, metres


def test_a_permuted_upload_gives_the_same_branches(gpu_ctx_factory, cases):
    """A small Y and a twig, uploaded again with the points of each permuted among themselves except the crack's lowest index
    (the start of CL4's first sweep, so that end a and with it every pos stay where they are): the same branches as point
    sets, the same tables, edges and summaries, and every id the lowest index of its branch under the new order."""
    ctx = _ctx(gpu_ctx_factory)
    y = cases["small_y1"][0]
    twig = cases["twig"][0] + np.array([0.0, 0.3, 0.0], np.float32)
    xyz = np.concatenate([y, twig]).astype(np.float32)
    k, ky = len(xyz), len(y)
    cloud, _ = _case_setup(ctx, xyz)
    first = ctx.crack_branches(1, RADIUS, STEP, 0.05)
    first_sk = ctx.crack_skeleton(1, RADIUS, STEP)
    ctx.crack_fuse_end()
    assert first["branch"][0] != -1 and first["branch"][ky] != -1, "the scene is wrong: a crack's first point is not credited"
    rng = np.random.default_rng(31)
    perm = np.concatenate([[0], 1 + rng.permutation(ky - 1), [ky], ky + 1 + rng.permutation(k - ky - 1)])
    assert sorted(perm.tolist()) == list(range(k)) and (perm != np.arange(k)).mean() > 0.9
    cloud2, _ = _case_setup(ctx, xyz[perm])
    second = ctx.crack_branches(1, RADIUS, STEP, 0.05)
    second_sk = ctx.crack_skeleton(1, RADIUS, STEP)
    ctx.crack_fuse_end()
    n = len(cloud)
    assert np.array_equal(cloud2[k:], cloud[k:])  # (the wall behind the points is the same)
    old_of = np.concatenate([perm, np.arange(k, n)])
    a, b = _named(first, first_sk, np.arange(n)), _named(second, second_sk, old_of)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]
    assert a[4].keys() == b[4].keys() and all(abs(a[4][key] - b[4][key]) <= 1e-9 * a[4][key] for key in a[4])
    own = [c for name, c in a[3].items() if name < k]
    assert (3, 0, 1, 3, 0, 0, 0) in own and any(c[:5] == (1, 0, 0, 2, 1) and c[5] >= 1 for c in own)  # the Y, and the twig pruned
    assert -2 in a[1].values() and -3 in a[1].values()
    inb = np.flatnonzero(second["branch"] >= 0)
    lowest = np.full(n, n, np.int64)
    np.minimum.at(lowest, second["branch"][inb], inb)
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
        return (L.pcp_crack_branches_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, None, None, C.byref(got)),
                L.pcp_crack_branch_edges_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, C.byref(got)),
                L.pcp_crack_branch_cracks_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, C.byref(got)))

    def skeleton_code():
        return L.pcp_crack_skeleton_nodes_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, None, C.byref(got))

    def directions_code():
        return L.pcp_crack_directions_fetch(ctx.h, C.c_int64(0), C.c_int64(1), None, None, C.byref(got))

    OK3, STATE3 = (capi.PCP_OK,) * 3, (capi.PCP_ERR_STATE,) * 3
    assert code(ctx.crack_branches) == capi.PCP_ERR_STATE  # CB9: no live fusion
    assert fetch_codes() == STATE3
    xyz = np.concatenate([cases["small_y1"][0], cases["uniform"][0][:700] + np.array([0.0, 0.2, 0.0], np.float32),
                          cases["twig"][0] - np.array([0.0, 0.3, 0.0], np.float32)]).astype(np.float32)
    cloud, poses, masks = _case_scene(xyz)
    cam = cw_ref.camera((64, 64))
    cam.update(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
    _setup(ctx, cam, cloud, poses, masks)
    assert code(ctx.crack_branches) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    none = ctx.crack_branches(1, RADIUS)  # zero crack points: success, no rows
    assert len(none["ids"]) == 0 and len(none["edge_branch"]) == 0 and len(none["cracks"]) == 0 and (none["branch"] == -1).all()
    assert fetch_codes() == OK3 and got.value == 0 and skeleton_code() == capi.PCP_OK
    w_max = cs_ref.w_max(RADIUS)
    below = float(np.float32((w_max - 1) * 2.0 ** -20))
    above = float(np.nextafter(np.float32(1024), np.float32(2048)))
    for mv, r, st, pr in ((0, 0.02, 0.04, 0.0), (4097, 0.02, 0.04, 0.0), (1, 0.004, 0.04, 0.0), (1, 1.5, 3.0, 0.0), (1, RADIUS, below, 0.0),
                          (1, RADIUS, 16.5, 0.0), (1, RADIUS, 0.0, 0.0), (1, RADIUS, float("nan"), 0.0), (1, RADIUS, STEP, above),
                          (1, RADIUS, STEP, -1e-30), (1, RADIUS, STEP, float("nan")), (1, RADIUS, STEP, float("inf"))):
        assert code(ctx.crack_branches, mv, r, st, pr) == capi.PCP_ERR_INVALID, (mv, r, st, pr)
    assert fetch_codes() == OK3  # (a refused call changes nothing)
    assert L.pcp_crack_branches(ctx.h, None, C.c_float(0.04), C.c_float(0.0), None, None, None) == capi.PCP_ERR_INVALID
    ctx.crack_fuse_add(0, 0, 150)
    assert fetch_codes() == STATE3  # an add ends the tables' life
    edge = ctx.crack_branches(1, RADIUS, STEP, 1024.0)  # CB1: 1024 is taken
    out = ctx.crack_branches(1, RADIUS, STEP, 0.05)
    kb, ke, kc = len(out["ids"]), len(out["edge_branch"]), len(out["cracks"])
    assert kb > kc > 10 and ke > 30 and out["pruned_branches"] > 0 and edge["pruned_branches"] >= out["pruned_branches"]
    # every output optional: the counts alone
    prm = capi.CrackLinkParams(1, RADIUS)
    a, b = C.c_int64(), C.c_int64()
    assert L.pcp_crack_branches(ctx.h, C.byref(prm), C.c_float(STEP), C.c_float(0.05), None, C.byref(a), C.byref(b)) == capi.PCP_OK
    assert (a.value, b.value) == (kb, out["pruned_branches"])
    assert L.pcp_crack_branches(ctx.h, C.byref(prm), C.c_float(STEP), C.c_float(0.05), None, None, None) == capi.PCP_OK
    # windows of the three tables
    for first, rows in ((0, 1), (3, 5), (kb - 2, 10), (kb, 4), (kb + 7, 4), (3, 0)):
        ids = np.full(rows, -7, np.int32)
        tab = np.full((rows, 15), -7, np.int64)
        mom = np.full((rows, 20), -7, np.int64)
        assert L.pcp_crack_branches_fetch(ctx.h, C.c_int64(first), C.c_int64(rows), capi._ptr(ids), capi._ptr(tab), capi._ptr(mom), C.byref(got)) == capi.PCP_OK
        g = got.value
        assert g == max(0, min(rows, kb - first))
        assert np.array_equal(ids[:g], out["ids"][first:first + g]) and np.array_equal(tab[:g], out["rows"][first:first + g])
        assert np.array_equal(mom[:g], out["moments"][first:first + g])
        assert (ids[g:] == -7).all() and (tab[g:] == -7).all() and (mom[g:] == -7).all()
    for first, rows in ((0, 1), (5, 9), (ke - 3, 10), (ke, 2), (ke + 5, 2), (2, 0)):
        tab = np.full(rows, -7, np.int32)
        assert L.pcp_crack_branch_edges_fetch(ctx.h, C.c_int64(first), C.c_int64(rows), capi._ptr(tab), C.byref(got)) == capi.PCP_OK
        g = got.value
        assert g == max(0, min(rows, ke - first)) and np.array_equal(tab[:g], out["edge_branch"][first:first + g]) and (tab[g:] == -7).all()
    for first, rows in ((0, 1), (4, 6), (kc - 1, 3), (kc, 2), (1, 0)):
        tab = np.full((rows, 7), -7, np.int64)
        assert L.pcp_crack_branch_cracks_fetch(ctx.h, C.c_int64(first), C.c_int64(rows), capi._ptr(tab), C.byref(got)) == capi.PCP_OK
        g = got.value
        assert g == max(0, min(rows, kc - first)) and np.array_equal(tab[:g], out["cracks"][first:first + g]) and (tab[g:] == -7).all()
    assert L.pcp_crack_branches_fetch(ctx.h, C.c_int64(-1), C.c_int64(1), None, None, None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branch_edges_fetch(ctx.h, C.c_int64(0), C.c_int64(-1), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branch_cracks_fetch(ctx.h, C.c_int64(-1), C.c_int64(0), None, None) == capi.PCP_ERR_INVALID
    # CB9 row by row.  Twice: the same bytes; components and directions keep the branches, and the branches keep the directions
    again = ctx.crack_branches(1, RADIUS, STEP, 0.05)
    assert all(out[key].tobytes() == again[key].tobytes() for key in cb_ref.KEYS)
    ctx.crack_components(1, 0.008)
    assert fetch_codes() == OK3
    ctx.crack_directions(1, 0.008)
    assert fetch_codes() == OK3 and directions_code() == capi.PCP_OK
    ctx.crack_branches(1, RADIUS, STEP, 0.05)
    assert directions_code() == capi.PCP_OK and skeleton_code() == capi.PCP_OK
    kept = ctx.crack_branches(1, RADIUS, STEP, 0.05)
    assert all(out[key].tobytes() == kept[key].tobytes() for key in cb_ref.KEYS)
    ctx.crack_skeleton(1, RADIUS, STEP)  # the skeleton is replaced: the branches made from the old one end
    assert fetch_codes() == STATE3 and skeleton_code() == capi.PCP_OK
    ctx.crack_branches(1, RADIUS, STEP, 0.05)
    ctx.crack_lengths(1, RADIUS)
    assert fetch_codes() == STATE3 and skeleton_code() == capi.PCP_ERR_STATE
    # the drops
    ctx.crack_branches(1, RADIUS, STEP, 0.05)
    ctx.crack_fuse_end()
    assert fetch_codes() == STATE3 and code(ctx.crack_branches) == capi.PCP_ERR_STATE
    ctx.crack_fuse_begin()
    ctx.crack_fuse_add(0, 0, 150)
    ctx.crack_branches(1, RADIUS, STEP, 0.05)
    ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
    assert fetch_codes() == STATE3 and code(ctx.crack_branches) == capi.PCP_ERR_STATE
    for drop in ("pcp_set_frames", "pcp_set_camera", "pcp_crack_fuse_begin"):  # the other rows of the table that drop them
        _setup(ctx, cam, cloud, poses, masks)
        ctx.crack_fuse_begin()
        ctx.crack_fuse_add(0, 0, 150)
        ctx.crack_branches(1, RADIUS, STEP, 0.05)
        assert fetch_codes() == OK3, drop
        if drop == "pcp_set_frames":
            ctx.set_frames(np.asarray(poses, np.float64))
        elif drop == "pcp_set_camera":
            ctx.set_camera(cam_struct(capi, cam), capi.default_cull_params())
        else:
            ctx.crack_fuse_begin()
        assert fetch_codes() == STATE3, drop


def test_nothing_else_moves(gpu_ctx_factory, small_scene):
    """the texels, a colour run, pcp_frame_visible, pcp_crack_width and the outputs of pcp_crack_components, _lengths, _skeleton
    and _directions are as without pcp_crack_branches in the cycle"""
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

    def cycle(with_branches):
        ctx.crack_fuse_begin()
        for f in (3, 2, 0):
            ctx.crack_fuse_add(f, 0, 150)
        state = ctx.crack_fuse_fetch()
        outs = []
        if with_branches:
            outs.append(ctx.crack_branches(1, 0.05, None, 0.2))
        comp = ctx.crack_components(1, 0.05)
        if with_branches:
            outs.append(ctx.crack_branches(1, 0.03, 0.2, 0.0))  # other parameters: its own tables
        directions = ctx.crack_directions(1, 0.05)
        lengths = ctx.crack_lengths(1, 0.05)
        if with_branches:
            outs.append(ctx.crack_branches(1, 0.05, None, 0.0))
        skeleton = ctx.crack_skeleton(1, 0.05)
        comp2 = ctx.crack_components(1, 0.05)
        assert all(np.asarray(comp[k]).tobytes() == np.asarray(comp2[k]).tobytes() for k in comp)
        state2 = ctx.crack_fuse_fetch()
        assert all(state[k].tobytes() == state2[k].tobytes() for k in state)
        ctx.crack_fuse_end()
        return state, comp, lengths, skeleton, directions, outs

    plain = cycle(False)
    with_it = cycle(True)
    outs = with_it[5]
    assert plain[1]["components"] >= 1 and len(outs[0]["cracks"]) == plain[1]["components"]
    for a, b in zip(plain[:5], with_it[:5]):
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    assert np.array_equal(ctx.download_result_packed(), packed)  # the colour result in place
    bgr1, mask1 = ctx.download_image(2)
    assert bgr0.tobytes() == bgr1.tobytes() and mask0.tobytes() == mask1.tobytes()
    vis1 = ctx.frame_visible(2)
    assert all(np.array_equal(vis0[k], vis1[k]) for k in vis0)
    cw1 = ctx.crack_width(2, 0, 150, want=("flags", "width"))
    assert cw0["flags"].tobytes() == cw1["flags"].tobytes() and cw0["width"].tobytes() == cw1["width"].tobytes()
    after = ctx.colorize()
    assert before["rgb"].tobytes() == after["rgb"].tobytes() and before["has"].tobytes() == after["has"].tobytes()
    # and the branches are the host form's under the fetched state, their points those of the components
    cloud = np.stack([s["x"], s["y"], s["z"]], axis=1).astype(np.float32)
    assert np.array_equal(outs[0]["branch"] != -1, plain[1]["label"] >= 0)
    if len(cloud) <= 65536:
        for out, (radius, step, prune) in list(zip(outs, ((0.05, None, 0.2), (0.03, 0.2, 0.0), (0.05, None, 0.0))))[:3 if plain[1]["crack_points"] <= 8000 else 1]:
            host = capi.crack_branches_host(cloud, plain[0]["views"], 1, radius, step, prune, plain[0]["sum_q"])
            cb_ref.assert_same(out, host, "small scene")
