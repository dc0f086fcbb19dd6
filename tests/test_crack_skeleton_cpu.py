"""CPU suite of the crack skeletons on the map (csrc/pcp_crack_skeleton.hpp through pcp_crack_skeleton_host: no context, no GPU)
against the restatement in _crack_skeleton_ref.py, by exact equality; and the restatement alone against topology it cannot
know: a band, an arc, Y and plus shapes, rings and a wall.

Measured with the restatement (test_known_topologies prints them), radius 5 mm: band 1.9929 m of skeleton at step 0.01 against
2.0065 m of geodesic length, arc 1.5645 m against 1.5715 m; Y (three arms of 0.6 m) 1.779-1.796 m of skeleton where the geodesic
length is 1.200-1.203 m; plus 2.369-2.390 m against 2.4 m of arms; ring of radius 0.3 m 1.884-1.886 m against 1.885 m, geodesic
0.944 m; small Y 35 nodes at step 0.01; the wall of 0.12 x 0.08 m comes out with 4 ends and 1 junction at every step."""
import os
import subprocess

import numpy as np
import pytest

import _crack_fuse_ref as ref
import _crack_skeleton_ref as cs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_crack_skeleton", "pcp_crack_skeleton_nodes_fetch", "pcp_crack_skeleton_edges_fetch", "pcp_crack_skeleton_cracks_fetch",
       "pcp_crack_skeleton_host")
RADIUS = 0.005
STEPS = (0.0075, 0.01, 0.02)
COMPONENT_NAMES = ["chain_shuffled", "chain_descending", "chains_touch", "chains_apart", "duplicates", "ring", "one_cell", "non_finite",
                   "min_views_1", "min_views_3", "single", "no_crack_point", "uniform"]
SHAPE_NAMES = ["band", "arc", "wall", "y1", "y2", "y3", "y4", "plus1", "plus2", "plus4", "ring1", "ring2", "ring3", "small_y1", "small_y2",
               "small_y3"]


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def cases():
    out = ref.component_cases(RADIUS)
    assert set(out) == set(COMPONENT_NAMES)
    shapes = cs_ref.shape_cases()
    assert set(shapes) == set(SHAPE_NAMES)
    for name, xyz in shapes.items():
        out[name] = (xyz, np.ones(len(xyz), np.uint32), 1)
    for xyz, views, _ in out.values():
        xyz.setflags(write=False)
        views.setflags(write=False)
    return out


_BASE, _WANT = {}, {}


def _sum_q(xyz, views):
    return (np.arange(len(xyz), dtype=np.uint64) * np.uint64(37)) % np.uint64(1000) * views.astype(np.uint64)


def _want(cases, name, step):
    """the restatement of a case at a step, computed once and left unchanged (pos and the links once per case)"""
    if (name, step) not in _WANT:
        xyz, views, min_views = cases[name]
        sum_q = _sum_q(xyz, views)
        if name not in _BASE:
            _BASE[name] = cs_ref.base(xyz, views, min_views, RADIUS, sum_q)
        res = cs_ref.skeleton(xyz, views, min_views, RADIUS, step, sum_q, _BASE[name])
        for v in res.values():
            v.setflags(write=False)
        _WANT[(name, step)] = res
    return _WANT[(name, step)]


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("name", COMPONENT_NAMES + SHAPE_NAMES)
def test_skeleton_host_equals_the_restatement(cases, name, step):
    capi = _capi()
    xyz, views, min_views = cases[name]
    want = _want(cases, name, step)
    got = capi.crack_skeleton_host(xyz, views, min_views, RADIUS, step, _sum_q(xyz, views))
    cs_ref.assert_same(got, want, f"{name} at {step}")
    cs_ref.check_rules(want, f"{name} at {step}")
    for k in cs_ref.METRES:  # CS7: both fp64 and correctly rounded
        assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k]), (name, step, k)
    cracks = want["cracks"]
    if name.startswith("chain_"):
        assert len(cracks) == 1 and cracks[0, 2:].tolist() == [2, 0, 0, 2] and cracks[0, 0] == want["nodes"][:, 1].max() + 1
    elif name == "chains_apart":
        assert len(cracks) == 2 and (cracks[:, 2] == 2).all() and not cracks[:, 3:5].any()
    elif name == "ring":
        assert len(cracks) == 1 and cracks[0, 2:5].tolist() == [0, 0, 1]
    elif name == "single":
        assert cracks.tolist() == [[1, 0, 0, 0, 0, 0]] and want["node"].tolist() == [0] and want["nodes"][0, :3].tolist() == [0, 0, 1]
    elif name == "no_crack_point":
        assert len(cracks) == 0 and len(want["ids"]) == 0 and len(want["edges"]) == 0 and (want["node"] == -1).all()
    elif name == "uniform":
        assert (cracks[:, 0] == 1).sum() > 10 and (cracks[:, 3] > 0).any()


@pytest.mark.parametrize("step", (0.01, 0.02))
def test_known_topologies(cases, step):
    """The shapes' ends, junctions and loops, and the skeleton length against the length of crack that is there -- what the
    geodesic length of the double sweep cannot say.  On the restatement alone."""
    def one(name):
        w = _want(cases, name, step)
        assert len(w["cracks"]) == 1, (name, "the cloud is not connected: keep the seed and the density")
        geodesic = _BASE[name]["lengths"]["rows"][0, 2] * cs_ref.UNIT
        c = w["cracks"][0]
        print(f"{name} at step {step}: nodes {c[0]} edges {c[1]} ends {c[2]} junctions {c[3]} loops {c[4]}, skeleton "
              f"{w['skeleton_length_m'][0]:.4f} m, geodesic {geodesic:.4f} m")
        return c, float(w["skeleton_length_m"][0]), geodesic

    for name in ("band", "arc"):
        c, length, geodesic = one(name)
        assert c[2:5].tolist() == [2, 0, 0] and 0.98 * geodesic < length <= geodesic
    for s in (1, 2, 3, 4):
        c, length, geodesic = one(f"y{s}")
        assert c[2:5].tolist() == [3, 1, 0] and abs(length - 1.8) < 0.02 * 1.8 and length > 1.4 * geodesic
    for s in (1, 2, 4):
        c, length, geodesic = one(f"plus{s}")
        assert c[2:5].tolist() == [4, 1, 0] and 2.34 <= length <= 2.40 and c[5] == 4
    for s in (1, 2, 3):
        c, length, geodesic = one(f"ring{s}")
        assert c[2:5].tolist() == [0, 0, 1] and c[0] == c[1] and abs(length - 2.0 * np.pi * 0.3) < 0.01 * 2.0 * np.pi * 0.3
        assert abs(geodesic - 0.944) < 0.002
        c, length, geodesic = one(f"small_y{s}")
        assert c[2:5].tolist() == [3, 1, 0] and (step != 0.01 or c[0] == 35)


def test_the_step_at_its_boundary_and_the_other_error_returns():
    capi = _capi()
    C = capi.C
    L = capi.load()
    xyz = np.zeros((4, 3), np.float32)
    views = np.ones(4, np.uint32)
    w_max = cs_ref.w_max(RADIUS)
    assert w_max == 5242
    at, below = np.float32(w_max * 2.0 ** -20), np.float32((w_max - 1) * 2.0 ** -20)
    assert cs_ref.step_q_of(at) == w_max and cs_ref.step_q_of(below) == w_max - 1
    assert capi.crack_skeleton_host(xyz, views, 1, RADIUS, float(at))["cracks"].tolist() == [[1, 0, 0, 0, 0, 0]]  # CS2: step_q = w_max
    assert len(capi.crack_skeleton_host(xyz, views, 1, RADIUS, 16.0)["ids"]) == 1
    for mv, r, st in ((1, RADIUS, float(below)), (1, RADIUS, float(np.nextafter(np.float32(16), np.float32(17)))), (1, RADIUS, 0.0),
                      (1, RADIUS, -0.01), (1, RADIUS, float("nan")), (1, 0.02, 0.019), (0, 0.02, 0.04), (4097, 0.02, 0.04), (1, 0.004, 0.04),
                      (1, 1.5, 3.0), (1, float("nan"), 0.04)):
        with pytest.raises(capi.PcpError) as e:
            capi.crack_skeleton_host(xyz, views, mv, r, st)
        assert e.value.code == capi.PCP_ERR_INVALID, (mv, r, st)
    assert len(capi.crack_skeleton_host(xyz, views, 1, 0.02)["ids"]) == 1  # the default step, 2 * radius
    far = np.array([[2.0e6, 0, 0], [0, 0, 0]], np.float32)
    with pytest.raises(capi.PcpError) as e:
        capi.crack_skeleton_host(far, np.ones(2, np.uint32), 1, RADIUS, 0.01)  # CS4: a crack point beyond 2^20 m
    assert e.value.code == capi.PCP_ERR_RANGE
    assert len(capi.crack_skeleton_host(far, np.array([0, 1], np.uint32), 1, RADIUS, 0.01)["ids"]) == 1  # ... but no crack point may lie there
    nul = [None] * 3
    args = (C.c_int32(1), C.c_float(0.02), C.c_float(0.04), None)
    assert L.pcp_crack_skeleton_host(C.c_int64(65537), capi._ptr(xyz), capi._ptr(views), *args, *nul, C.c_int64(0), None, None, *nul) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_skeleton_host(C.c_int64(4), None, capi._ptr(views), *args, *nul, C.c_int64(0), None, None, *nul) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_skeleton_host(C.c_int64(-1), None, None, *args, *nul, C.c_int64(0), None, None, *nul) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_skeleton_host(C.c_int64(4), capi._ptr(xyz), capi._ptr(views), *args, *nul, C.c_int64(-1), None, None, *nul) == capi.PCP_ERR_INVALID
    kn, ke, kc = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert L.pcp_crack_skeleton_host(C.c_int64(0), None, None, *args, *nul, C.c_int64(0), None, None, C.byref(kn), C.byref(ke), C.byref(kc)) == capi.PCP_OK
    assert (kn.value, ke.value, kc.value) == (0, 0, 0)
    assert L.pcp_crack_skeleton_host(C.c_int64(4), capi._ptr(xyz), capi._ptr(views), *args, *nul, C.c_int64(0), None, None, C.byref(kn), C.byref(ke), C.byref(kc)) == capi.PCP_OK
    assert (kn.value, ke.value, kc.value) == (1, 0, 1)  # four coincident points: one node, every output optional
    with pytest.raises(ValueError):
        capi.crack_skeleton_host(xyz, views[:3])
    with pytest.raises(ValueError):
        capi.crack_skeleton_host(xyz, views, sum_q=np.zeros(3, np.uint64))
    # no context
    assert L.pcp_crack_skeleton(None, None, C.c_float(0.04), None, None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_skeleton_nodes_fetch(None, C.c_int64(0), C.c_int64(0), None, None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_skeleton_edges_fetch(None, C.c_int64(0), C.c_int64(0), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_skeleton_cracks_fetch(None, C.c_int64(0), C.c_int64(0), None, None) == capi.PCP_ERR_INVALID


def test_the_edge_capacity_is_a_window_and_the_count_is_whole(cases):
    capi = _capi()
    C = capi.C
    L = capi.load()
    xyz, views, _ = cases["small_y1"]
    want = _want(cases, "small_y1", 0.01)
    e = len(want["edges"])
    assert e == 34
    some = np.full((10, 3), -7, np.int64)
    ke = C.c_int64()
    rc = L.pcp_crack_skeleton_host(C.c_int64(len(xyz)), capi._ptr(xyz), capi._ptr(views), C.c_int32(1), C.c_float(RADIUS), C.c_float(0.01), None,
                                   None, None, None, C.c_int64(9), capi._ptr(some), None, None, C.byref(ke), None)
    assert rc == capi.PCP_OK and ke.value == e and np.array_equal(some[:9], want["edges"][:9]) and (some[9] == -7).all()


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    assert callable(capi.Context.crack_skeleton) and callable(capi.crack_skeleton_host) and callable(capi.crack_skeleton_metres)
    assert lib.pcp_abi_version() == 6 and capi.K_COUNT == 13
    assert len(capi.CS_NODE) == 10 and len(capi.CS_EDGE) == 3 and len(capi.CS_CRACK) == 6
    assert capi.crack_skeleton_step(0.005) == float(np.float32(0.01))


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  ' + "\n  ".join(f"(void){s};" for s in NEW) +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["crack_skeleton_selftest"]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "crack_skeleton_selftest.cpp")
    exe = str(tmp_path / "crack_skeleton_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_pipeline_refuses_index_shards():
    from pointcloudprocessor_amd import pipeline

    with pytest.raises(ValueError) as e:
        pipeline.PointCloudColorizer(None, rank=0, world=2).crack_map(skeleton=True)
    assert "index shard" in str(e.value) and "not built" in str(e.value)
