"""CPU suite of the crack branches on the map (csrc/pcp_crack_branch.hpp through pcp_crack_branches_host: no context, no GPU)
against the restatement in _crack_branch_ref.py, by exact equality; the restatement alone against what CB3, CB6 and CB7 promise
and against topology it cannot know: a band, an arc, Y and plus shapes, rings, and a stem with a side twig.

Measured with the restatement (test_known_answers prints them), radius 5 mm, steps 0.01 and 0.02, prune 0 and 0.05: the axis of
a branch of Y (three arms of 0.6 m, seeds 1-4) is at most 0.875 degrees off its arm, within half of the directions suite's 2
degrees, so the bar is 2 degrees (small Y, arms of 0.12 m: 1.235 degrees, not asserted); the three branch lengths of Y and no
bridge add up to skeleton_length_m to 6e-16 relative.  twig (seed 1): three branches, at prune 0.05 one, the twig's 2 nodes (1
at step 0.02) and 37 points (13) pruned.  twig_at_end (seed 3): the twig holds end b and stays; the stub of 15 mm the stem has
left past it goes instead -- in a tree end a and end b are the ends of a longest way, so a twig shorter than both sides of the
stem cannot hold one, and what is left of the stem past a twig that does is shorter than the twig: three branches at prune 0,
one at 0.05 with the twig's points in it."""
import os
import subprocess

import numpy as np
import pytest

import _crack_branch_ref as cb_ref
import _crack_direction_ref as cd_ref
import _crack_fuse_ref as ref
import _crack_skeleton_ref as cs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_crack_branches", "pcp_crack_branches_fetch", "pcp_crack_branch_edges_fetch", "pcp_crack_branch_cracks_fetch",
       "pcp_crack_branches_host", "pcp_crack_branch_lengths_host")
RADIUS = 0.005
STEPS = (0.01, 0.02)
PRUNES = (0.0, 0.05)
COMPONENT_NAMES = ["chain_shuffled", "chain_descending", "chains_touch", "chains_apart", "duplicates", "ring", "one_cell", "non_finite",
                   "min_views_1", "min_views_3", "single", "no_crack_point", "uniform"]
SHAPE_NAMES = ["band", "arc", "wall", "y1", "y2", "y3", "y4", "plus1", "plus2", "plus4", "ring1", "ring2", "ring3", "small_y1", "small_y2",
               "small_y3"]
NEW_NAMES = ["twig", "twig_at_end"]
Y_BAR_DEG = 2.0  # the directions suite's; the restatement's worst is 0.875 (module docstring)


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def cases():
    out = ref.component_cases(RADIUS)
    assert set(out) == set(COMPONENT_NAMES)
    shapes = cs_ref.shape_cases()
    assert set(shapes) == set(SHAPE_NAMES)
    shapes.update(cb_ref.new_cases())
    for name, xyz in shapes.items():
        out[name] = (xyz, np.ones(len(xyz), np.uint32), 1)
    for xyz, views, _ in out.values():
        xyz.setflags(write=False)
        views.setflags(write=False)
    return out


_BASE, _SKEL, _WANT = {}, {}, {}


def _sum_q(xyz, views):
    return (np.arange(len(xyz), dtype=np.uint64) * np.uint64(37)) % np.uint64(1000) * views.astype(np.uint64)


def _want(cases, name, step, prune):
    """the restatement of a case, computed once and left unchanged (pos and the links once per case, the diagram once per step)"""
    if (name, step, prune) not in _WANT:
        xyz, views, min_views = cases[name]
        sum_q = _sum_q(xyz, views)
        if name not in _BASE:
            _BASE[name] = cs_ref.base(xyz, views, min_views, RADIUS, sum_q)
        if (name, step) not in _SKEL:
            _SKEL[(name, step)] = cs_ref.skeleton(xyz, views, min_views, RADIUS, step, sum_q, _BASE[name])
        res = cb_ref.branches(xyz, views, min_views, RADIUS, step, prune, sum_q, _BASE[name], _SKEL[(name, step)])
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WANT[(name, step, prune)] = res
    return _WANT[(name, step, prune)]


@pytest.mark.parametrize("prune", PRUNES)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("name", COMPONENT_NAMES + SHAPE_NAMES + NEW_NAMES)
def test_branches_host_equals_the_restatement(cases, name, step, prune):
    capi = _capi()
    xyz, views, min_views = cases[name]
    want = _want(cases, name, step, prune)
    got = capi.crack_branches_host(xyz, views, min_views, RADIUS, step, prune, _sum_q(xyz, views))
    cb_ref.assert_same(got, want, f"{name} at {step}, prune {prune}")  # (CB8's doubles included)
    cb_ref.check_rules(want, prune, f"{name} at {step}, prune {prune}")
    # axes and anisotropies against eigh at the bar of the directions suite, the same eigen-gap exemption
    eig = cd_ref.axis_of_rows(want["moments"])
    assert np.array_equal(got["link_count"], eig["link_count"]), name
    has = eig["axis"].any(axis=1)
    assert np.array_equal(got["axis"].any(axis=1), has), (name, "axis validity")
    check = has & ~(eig["axis_gap"] < 1e-3)
    cd_ref._close(got["axis"][check], got["anisotropy"][check], eig["axis"][check], eig["axis_anisotropy"][check], f"{name} at {step}, {prune}:")
    rows, cracks = want["rows"], want["cracks"]
    if name.startswith("chain_") or name in ("band", "arc"):
        assert len(rows) == 1 and rows[0, 3] == 0 and rows[0, 2] == rows[0, 1] - 1 and cracks[0].tolist() == [1, 0, 0, 2, 0, 0, 0]
    elif name == "chains_apart":
        assert len(rows) == 2 and not rows[:, 3].any()
    elif name in ("ring", "ring1", "ring2", "ring3"):
        assert len(rows) == 1 and rows[0, 3] == 0 and rows[0, 2] == rows[0, 1] and cracks[0].tolist() == [1, 0, 0, 0, 0, 0, 0]
    elif name == "single":
        assert rows[0, :7].tolist() == [0, 1, 0, 0, -1, -1, 1] and want["branch"].tolist() == [0]
    elif name == "no_crack_point":
        assert len(rows) == 0 and len(cracks) == 0 and len(want["edge_branch"]) == 0 and (want["branch"] == -1).all()


@pytest.mark.parametrize("step", STEPS)
def test_known_answers(cases, step):
    """the issue's table, on the restatement alone"""
    def one(name, prune):
        w = _want(cases, name, step, prune)
        assert len(w["cracks"]) == 1, (name, "the cloud is not connected: keep the seed and the density")
        print(f"{name} at step {step}, prune {prune}: branches {len(w['ids'])} nodes {w['rows'][:, 1].tolist()} attachments "
              f"{w['rows'][:, 3].tolist()} crack {w['cracks'][0].tolist()}")
        return w, w["rows"], w["cracks"][0]

    for name in ("band", "arc"):
        _, rows, c = one(name, 0.0)
        assert len(rows) == 1 and rows[0, 3] == 0
    for name, arms in [(f"small_y{s}", 3) for s in (1, 2, 3)] + [(f"y{s}", 3) for s in (1, 2, 3, 4)] + [(f"plus{s}", 4) for s in (1, 2, 4)]:
        _, rows, c = one(name, 0.0)
        assert len(rows) == arms and (rows[:, 3] == 1).all() and (rows[:, 4] == rows[0, 4]).all() and (rows[:, 5] == -1).all(), name
        assert c.tolist() == [arms, 0, 1, arms, 0, 0, 0], name
    for s in (1, 2, 3):
        _, rows, c = one(f"ring{s}", 0.0)
        assert len(rows) == 1 and rows[0, 3] == 0 and rows[0, 2] == rows[0, 1]
    _, rows, c = one("twig", 0.0)
    assert len(rows) == 3 and c.tolist() == [3, 0, 1, 3, 0, 0, 0]
    w, rows, c = one("twig", 0.05)
    assert len(rows) == 1 and c[4] == 1 and c[2] == 0 and c[3] == 2 and c[5] >= 1 and c[6] > 0
    xyz = cases["twig"][0]
    pruned = w["branch"] == cb_ref.PRUNED
    assert pruned.sum() == c[6] and (xyz[pruned, 1] > 0.002).all() and not pruned[:600].any(), "the pruned points are the twig's"
    assert w["kept_length_m"][0] < w["skeleton"]["skeleton_length_m"][0] and w["length_m"][0] == w["kept_length_m"][0]
    # twig_at_end: the twig holds end b (its tip is the longest way from end a) and is never a spur; see the module docstring
    w, rows, c = one("twig_at_end", 0.0)
    assert len(rows) == 3 and c.tolist() == [3, 0, 1, 3, 0, 0, 0]
    end_b = int(w["lengths"]["rows"][0, 1])
    assert end_b >= 600 and cases["twig_at_end"][0][end_b, 1] > 0.025, "the scene is wrong: end b is not the twig's tip"
    twig_branch = int(np.flatnonzero(w["ids"] == w["branch"][end_b])[0])
    assert rows[twig_branch, 3] == 1 and rows[twig_branch, 1] * cs_ref.step_q_of(step) < cb_ref.prune_q_of(0.05), "short enough to go, but for its end"
    w, rows, c = one("twig_at_end", 0.05)
    assert (w["branch"][600:] >= 0).all() and w["branch"][end_b] >= 0, "the twig is kept"
    gone = w["branch"] == cb_ref.PRUNED
    assert c[4] == 1 and gone.any() and (cases["twig_at_end"][0][gone, 0] > 0.225).all() and not gone[600:].any(), "the stub past the twig goes"
    assert len(rows) == 1 and c[2] == 0 and c[3] == 2


@pytest.mark.parametrize("prune", PRUNES)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("seed", (1, 2, 3, 4))
def test_the_branches_of_y(cases, seed, step, prune):
    """the three lengths add up, with the bridges, to the skeleton's; each branch's axis lies along its arm"""
    capi = _capi()
    w = _want(cases, f"y{seed}", step, prune)
    sk = w["skeleton"]
    assert len(w["ids"]) == 3 and not (w["edge_branch"] == cb_ref.EDGE_PRUNED).any()
    total = w["length_m"].sum() + sk["edge_length_m"][w["edge_branch"] == cb_ref.BRIDGE].sum()
    assert abs(total - sk["skeleton_length_m"][0]) <= 1e-9 * sk["skeleton_length_m"][0]
    assert abs(w["kept_length_m"][0] - sk["skeleton_length_m"][0]) <= 1e-9 * sk["skeleton_length_m"][0]
    arms = cd_ref.ypsilon_arms()
    arm = np.argmax(w["centroid"][:, :2] @ arms[:, :2].T, axis=1)
    assert sorted(arm.tolist()) == [0, 1, 2]
    for what, axes in (("restatement", cd_ref.axis_of_rows(w["moments"])["axis"]), ("library", capi.crack_axis_host(w["moments"])["axis"])):
        ang = [float(cd_ref.angle_deg(axes[b], arms[arm[b]])[0]) for b in range(3)]
        print(f"y{seed} at step {step}, prune {prune}, {what}: degrees off the arm {ang}")
        assert max(ang) <= Y_BAR_DEG, (what, ang)
    assert (np.abs(w["length_m"] - 0.6) < 0.03).all() and (w["mean_width"] > 0).all()
    assert (np.abs(np.linalg.norm(w["centroid"][:, :2], axis=1) - 0.3) < 0.02).all()


def test_prune_at_its_boundary_and_the_other_error_returns():
    capi = _capi()
    C = capi.C
    L = capi.load()
    xyz = np.zeros((4, 3), np.float32)
    views = np.ones(4, np.uint32)
    for prune in (0.0, 1024.0):  # CB1: both ends are taken
        out = capi.crack_branches_host(xyz, views, 1, RADIUS, 0.01, prune)
        assert out["cracks"].tolist() == [[1, 0, 0, 0, 0, 0, 0]] and out["rows"][0, :7].tolist() == [0, 1, 0, 0, -1, -1, 4]
    w_max = cs_ref.w_max(RADIUS)
    below = float(np.float32((w_max - 1) * 2.0 ** -20))
    above = float(np.nextafter(np.float32(1024), np.float32(2048)))
    for mv, r, st, pr in ((1, RADIUS, 0.01, above), (1, RADIUS, 0.01, -1e-30), (1, RADIUS, 0.01, float("nan")), (1, RADIUS, 0.01, float("inf")),
                          (1, RADIUS, 0.01, -float("inf")), (1, RADIUS, below, 0.0), (1, RADIUS, 16.5, 0.0), (1, RADIUS, 0.0, 0.0),
                          (1, RADIUS, float("nan"), 0.0), (1, 0.02, 0.019, 0.0), (0, 0.02, 0.04, 0.0), (4097, 0.02, 0.04, 0.0), (1, 0.004, 0.04, 0.0),
                          (1, 1.5, 3.0, 0.0), (1, float("nan"), 0.04, 0.0)):
        with pytest.raises(capi.PcpError) as e:
            capi.crack_branches_host(xyz, views, mv, r, st, pr)
        assert e.value.code == capi.PCP_ERR_INVALID, (mv, r, st, pr)
        assert "pcp_crack_branches_host" in str(e.value)
    assert len(capi.crack_branches_host(xyz, views, 1, 0.02)["ids"]) == 1  # the default step, 2 * radius
    far = np.array([[2.0e6, 0, 0], [0, 0, 0]], np.float32)
    with pytest.raises(capi.PcpError) as e:
        capi.crack_branches_host(far, np.ones(2, np.uint32), 1, RADIUS, 0.01)  # CS4's refusal: a crack point beyond 2^20 m
    assert e.value.code == capi.PCP_ERR_RANGE
    assert len(capi.crack_branches_host(far, np.array([0, 1], np.uint32), 1, RADIUS, 0.01)["ids"]) == 1
    args = (C.c_int32(1), C.c_float(0.02), C.c_float(0.04), C.c_float(0.0), None)
    nul4, nul3 = [None] * 4, [None] * 3
    assert L.pcp_crack_branches_host(C.c_int64(65537), capi._ptr(xyz), capi._ptr(views), *args, *nul4, C.c_int64(0), None, None, *nul3) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branches_host(C.c_int64(4), None, capi._ptr(views), *args, *nul4, C.c_int64(0), None, None, *nul3) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branches_host(C.c_int64(-1), None, None, *args, *nul4, C.c_int64(0), None, None, *nul3) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branches_host(C.c_int64(4), capi._ptr(xyz), capi._ptr(views), *args, *nul4, C.c_int64(-1), None, None, *nul3) == capi.PCP_ERR_INVALID
    kb, ke, kc = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert L.pcp_crack_branches_host(C.c_int64(0), None, None, *args, *nul4, C.c_int64(0), None, None, C.byref(kb), C.byref(ke), C.byref(kc)) == capi.PCP_OK
    assert (kb.value, ke.value, kc.value) == (0, 0, 0)
    assert L.pcp_crack_branches_host(C.c_int64(4), capi._ptr(xyz), capi._ptr(views), *args, *nul4, C.c_int64(0), None, None, C.byref(kb), C.byref(ke), C.byref(kc)) == capi.PCP_OK
    assert (kb.value, ke.value, kc.value) == (1, 0, 1)  # four coincident points: one branch, every output optional
    with pytest.raises(ValueError):
        capi.crack_branches_host(xyz, views[:3])
    with pytest.raises(ValueError):
        capi.crack_branches_host(xyz, views, sum_q=np.zeros(3, np.uint64))
    # no context
    assert L.pcp_crack_branches(None, None, C.c_float(0.04), C.c_float(0.0), None, None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branches_fetch(None, C.c_int64(0), C.c_int64(0), None, None, None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branch_edges_fetch(None, C.c_int64(0), C.c_int64(0), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branch_cracks_fetch(None, C.c_int64(0), C.c_int64(0), None, None) == capi.PCP_ERR_INVALID


def test_the_lengths_entry_refuses_rows_that_name_nothing(cases):
    """pcp_crack_branch_lengths_host (CB8, the one expression of every host layer; the equality test above compares its doubles
    with the restatement's): a row that names a node, a branch or a crack that is not there is PCP_ERR_INVALID"""
    capi = _capi()
    C = capi.C
    L = capi.load()
    want = _want(cases, "small_y1", 0.01, 0.0)
    sk = want["skeleton"]
    nodes, edges, eb = np.ascontiguousarray(sk["nodes"]), np.ascontiguousarray(sk["edges"]), np.ascontiguousarray(want["edge_branch"])
    B, K = len(want["ids"]), len(want["cracks"])

    def call(nodes, edges, eb, b=B, k=K):
        length, kept = np.full(max(b, 0), -7.0), np.full(k, -7.0)
        rc = L.pcp_crack_branch_lengths_host(C.c_int64(len(nodes)), capi._ptr(nodes), C.c_int64(len(edges)), capi._ptr(edges), capi._ptr(eb),
                                             C.c_int64(b), C.c_int64(k), capi._ptr(length), capi._ptr(kept))
        return rc, length, kept

    rc, length, kept = call(nodes, edges, eb)
    assert rc == capi.PCP_OK and np.array_equal(length, want["length_m"]) and np.array_equal(kept, want["kept_length_m"])
    for col, value in ((0, len(nodes)), (1, -1)):
        bad = edges.copy()
        bad[3, col] = value
        assert call(nodes, bad, eb)[0] == capi.PCP_ERR_INVALID
    bad = eb.copy()
    bad[0] = B
    assert call(nodes, edges, bad)[0] == capi.PCP_ERR_INVALID
    for col, value in ((0, K), (2, 0)):
        bad = nodes.copy()
        bad[1, col] = value
        assert call(bad, edges, eb)[0] == capi.PCP_ERR_INVALID
    assert call(nodes, edges, eb, b=-1)[0] == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branch_lengths_host(C.c_int64(len(nodes)), None, C.c_int64(0), None, None, C.c_int64(0), C.c_int64(0), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_branch_lengths_host(C.c_int64(0), None, C.c_int64(0), None, None, C.c_int64(0), C.c_int64(0), None, None) == capi.PCP_OK


def test_the_edge_capacity_is_a_window_and_the_count_is_whole(cases):
    capi = _capi()
    C = capi.C
    L = capi.load()
    xyz, views, _ = cases["small_y1"]
    want = _want(cases, "small_y1", 0.01, 0.0)
    e = len(want["edge_branch"])
    assert e == 34
    some = np.full(10, -7, np.int32)
    ke = C.c_int64()
    rc = L.pcp_crack_branches_host(C.c_int64(len(xyz)), capi._ptr(xyz), capi._ptr(views), C.c_int32(1), C.c_float(RADIUS), C.c_float(0.01), C.c_float(0.0),
                                   None, None, None, None, None, C.c_int64(9), capi._ptr(some), None, None, C.byref(ke), None)
    assert rc == capi.PCP_OK and ke.value == e and np.array_equal(some[:9], want["edge_branch"][:9]) and some[9] == -7


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    assert callable(capi.Context.crack_branches) and callable(capi.crack_branches_host) and callable(capi.crack_branches_metres)
    assert lib.pcp_abi_version() == 6 and capi.K_COUNT == 13
    assert len(capi.CB_ROW) == 15 and len(capi.CB_CRACK) == 7
    assert (capi.CB_NO_POINT, capi.CB_JUNCTION, capi.CB_PRUNED, capi.CB_BRIDGE, capi.CB_EDGE_PRUNED) == (-1, -2, -3, -1, -2)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  ' + "\n  ".join(f"(void){s};" for s in NEW) +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["crack_branch_selftest"]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "crack_branch_selftest.cpp")
    exe = str(tmp_path / "crack_branch_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_pipeline_refuses_index_shards():
    from pointcloudprocessor_amd import pipeline

    with pytest.raises(ValueError) as e:
        pipeline.PointCloudColorizer(None, rank=0, world=2).crack_map(branches=True)
    assert "index shard" in str(e.value) and "not built" in str(e.value)
