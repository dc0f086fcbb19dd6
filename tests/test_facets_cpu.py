"""CPU suite of the planar facets (csrc/pcp_facets.hpp through pcp_facets_host and pcp_facet_plane_host: no context, no GPU)
against the restatement in _facets_ref.py, by exact equality of labels, ids, the ten integers and the boxes; shapes whose
partition is known; the refusals, the ABI and the stand-alone self-test plain and under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _facets_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_facets", "pcp_facets_fetch", "pcp_facets_host", "pcp_facet_plane_host", "pcp_ortho_add_facet")
SCENE = dict(link_radius=0.5, angle_deg=10.0, plane_tol=0.01, max_curvature=0.01, min_points=50)


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def scene():
    """synth.make_cloud(20000) with numpy normals at r = 0.5, and its restatement: computed once, left unchanged"""
    from pointcloudprocessor_amd import synth

    x, y, z, _ = synth.make_cloud(20000)
    xyz = np.stack([x, y, z], axis=1).astype(np.float32)
    normal, curv = ref.numpy_normals(xyz, 0.5)
    want = ref.facets(xyz, normal, curv, **SCENE)
    for a in (xyz, normal, curv, *[v for v in want.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return dict(xyz=xyz, normal=normal, curv=curv, want=want)


def _same(got, want):
    assert np.array_equal(got["label"], want["label"])
    assert np.array_equal(got["ids"], want["ids"])
    assert np.array_equal(got["rows"], want["rows"])
    assert got["box"].tobytes() == want["box"].tobytes()


def test_host_equals_the_restatement_on_the_scene(scene):
    capi = _capi()
    got = capi.facets_host(scene["xyz"], scene["normal"], scene["curv"], **SCENE)
    want = scene["want"]
    print("facets", want["facets"], "components", want["components"], "facet points", want["facet_points"], "largest", want["rows"][:, 0].max())
    assert want["facets"] >= 6 and want["facet_points"] > 10000  # (the scene is not degenerate: the room's six faces at least)
    _same(got, want)


def test_negating_half_of_the_normals_changes_nothing(scene):
    capi = _capi()
    rng = np.random.default_rng(5)
    flip = rng.random(len(scene["xyz"])) < 0.5
    normal = scene["normal"].copy()
    normal[flip] = -normal[flip]
    _same(capi.facets_host(scene["xyz"], normal, scene["curv"], **SCENE), scene["want"])


def test_the_partition_is_the_same_under_a_permutation(scene):
    capi = _capi()
    n = len(scene["xyz"])
    perm = np.random.default_rng(6).permutation(n)  # new row k = old row perm[k]
    got = capi.facets_host(scene["xyz"][perm], scene["normal"][perm], scene["curv"][perm], **SCENE)
    old = scene["want"]["label"]
    # a facet's id in the new order is the lowest NEW index of its members: map the old labels across and compare
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    want = np.full(n, -1, np.int64)
    in_facet = old[perm] >= 0
    lowest = np.full(n, n, np.int64)
    np.minimum.at(lowest, old[perm][in_facet], np.flatnonzero(in_facet))
    want[in_facet] = lowest[old[perm][in_facet]]
    assert np.array_equal(got["label"], want)
    assert np.array_equal(np.sort(got["rows"][:, 0]), np.sort(scene["want"]["rows"][:, 0]))


def _sheet(rng, m, z=0.0, tilt_deg=0.0, x0=0.0):
    a, b = rng.random(m), rng.random(m)
    t = np.deg2rad(tilt_deg)
    xyz = np.stack([x0 + a * np.cos(t), b, z + a * np.sin(t)], axis=1).astype(np.float32)
    normal = np.tile(np.array([-np.sin(t), 0.0, np.cos(t)], np.float32), (m, 1))
    return xyz, normal


def test_two_parallel_sheets_three_centimetres_apart():
    capi = _capi()
    rng = np.random.default_rng(7)
    a, na = _sheet(rng, 4000)
    b, nb = _sheet(rng, 4000, z=0.03)
    xyz, normal = np.concatenate([a, b]), np.concatenate([na, nb])
    curv = np.zeros(len(xyz), np.float32)
    prm = dict(link_radius=0.05, angle_deg=10.0, max_curvature=0.02, min_points=1000)
    two = capi.facets_host(xyz, normal, curv, plane_tol=0.01, **prm)
    one = capi.facets_host(xyz, normal, curv, plane_tol=0.05, **prm)
    assert len(two["ids"]) == 2 and sorted(two["rows"][:, 0]) == [4000, 4000]
    assert len(np.unique(two["label"][:4000])) == 1 and len(np.unique(two["label"][4000:])) == 1
    assert len(one["ids"]) == 1 and one["rows"][0, 0] == 8000
    _same(two, ref.facets(xyz, normal, curv, plane_tol=0.01, **prm))
    _same(one, ref.facets(xyz, normal, curv, plane_tol=0.05, **prm))


def test_a_sheet_folded_by_twenty_degrees():
    capi = _capi()
    rng = np.random.default_rng(8)
    a, na = _sheet(rng, 4000, x0=-1.0)           # x in [-1, 0], flat
    b, nb = _sheet(rng, 4000, tilt_deg=20.0)     # from the fold at x = 0 upwards
    xyz, normal = np.concatenate([a, b]), np.concatenate([na, nb])
    curv = np.zeros(len(xyz), np.float32)
    prm = dict(link_radius=0.05, plane_tol=0.05, max_curvature=0.02, min_points=1000)
    two = capi.facets_host(xyz, normal, curv, angle_deg=10.0, **prm)
    one = capi.facets_host(xyz, normal, curv, angle_deg=30.0, **prm)
    assert len(two["ids"]) == 2 and sorted(two["rows"][:, 0]) == [4000, 4000]
    assert len(one["ids"]) == 1 and one["rows"][0, 0] == 8000
    _same(two, ref.facets(xyz, normal, curv, angle_deg=10.0, **prm))


def test_a_sphere_is_one_component_and_not_planar():
    capi = _capi()
    rng = np.random.default_rng(9)
    d = rng.normal(size=(6000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (np.array([2.0, -1.0, 3.0]) + 0.5 * d).astype(np.float32)
    got = capi.facets_host(xyz, d.astype(np.float32), np.zeros(len(xyz), np.float32), link_radius=0.06, angle_deg=10.0, plane_tol=0.01,
                           max_curvature=0.02, min_points=1000)
    assert len(got["ids"]) == 1 and got["rows"][0, 0] == 6000 and got["ids"][0] == 0  # the local rule walks round the sphere
    plane = capi.facet_plane_host(xyz[0], got["rows"][0])
    assert plane[6] > 0.1  # ... and the global test flags it: rms of a 0.5 m sphere about any plane is ~0.29 m
    assert np.abs(plane[:3] - np.array([2.0, -1.0, 3.0])).max() < 0.02


def test_min_points_on_both_sides_of_a_component(scene):
    capi = _capi()
    want = scene["want"]
    size = int(np.sort(want["rows"][:, 0])[len(want["ids"]) // 2])
    fid = int(want["ids"][np.flatnonzero(want["rows"][:, 0] == size)[0]])
    prm = dict(SCENE)
    prm["min_points"] = size
    at = capi.facets_host(scene["xyz"], scene["normal"], scene["curv"], **prm)
    prm["min_points"] = size + 1
    above = capi.facets_host(scene["xyz"], scene["normal"], scene["curv"], **prm)
    assert fid in at["ids"] and (at["label"] == fid).sum() == size
    assert fid not in above["ids"] and (above["label"] == fid).sum() == 0
    assert (above["label"][want["label"] == fid] == -1).all()


def test_plane_against_eigh(scene):
    capi = _capi()
    want = scene["want"]
    checked = 0
    for fid, row in zip(want["ids"], want["rows"]):
        got = capi.facet_plane_host(scene["xyz"][fid], row)
        exp = ref.plane(scene["xyz"][fid], row)
        print(fid, int(row[0]), "rms", got[6], exp[6], "normal diff", np.abs(got[3:6] - exp[3:6]).max())
        assert np.allclose(got[:3], exp[:3], rtol=1e-9, atol=0.0)
        assert abs(got[6] - exp[6]) <= 1e-9 * exp[6]
        assert np.abs(got[3:6] - exp[3:6]).max() <= 1e-6
        assert abs(np.linalg.norm(got[3:6]) - 1.0) < 1e-12 and got[3 + np.argmax(np.abs(got[3:6]))] > 0
        checked += 1
    assert checked >= 6


def test_refusals():
    capi = _capi()
    xyz = np.zeros((4, 3), np.float32)
    normal = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    curv = np.zeros(4, np.float32)
    good = dict(link_radius=0.1, angle_deg=10.0, plane_tol=0.01, max_curvature=0.02, min_points=1)
    assert len(capi.facets_host(xyz, normal, curv, **good)["ids"]) == 1
    for key, value in (("link_radius", 0.004), ("link_radius", 1.5), ("angle_deg", 0.0), ("angle_deg", 46.0), ("plane_tol", 5e-5),
                       ("plane_tol", 0.2), ("max_curvature", -1.0), ("max_curvature", float("nan")), ("min_points", 0),
                       ("min_points", (1 << 24) + 1)):
        with pytest.raises(capi.PcpError) as e:
            capi.facets_host(xyz, normal, curv, **{**good, key: value})
        assert e.value.code == capi.PCP_ERR_INVALID and key in str(e.value), (key, value, str(e.value))
    big = np.zeros((65537, 3), np.float32)
    with pytest.raises(capi.PcpError) as e:
        capi.facets_host(big, big, np.zeros(65537, np.float32), **good)
    assert e.value.code == capi.PCP_ERR_INVALID and "65536" in str(e.value)
    with pytest.raises(capi.PcpError) as e:
        capi.facet_plane_host(np.zeros(3, np.float32), np.zeros(10, np.int64))
    assert e.value.code == capi.PCP_ERR_INVALID
    L = capi.load()
    assert L.pcp_facets_host(C.c_int64(4), None, None, None, C.byref(capi.FacetParams(0.1, 10.0, 0.01, 0.02, 1)), None, None, None, None,
                             None) == capi.PCP_ERR_INVALID
    assert L.pcp_facets_host(C.c_int64(0), None, None, None, None, None, None, None, None, None) == capi.PCP_ERR_INVALID
    # no facet point at all, and an empty cloud
    none = capi.facets_host(xyz, np.zeros((4, 3), np.float32), curv, **good)
    assert len(none["ids"]) == 0 and (none["label"] == -1).all()
    assert len(capi.facets_host(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), **good)["ids"]) == 0


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    assert callable(capi.Context.facets) and callable(capi.Context.facets_fetch) and callable(capi.Context.ortho_add_facet)
    assert callable(capi.facets_host) and callable(capi.facet_plane_host)
    assert lib.pcp_abi_version() == 6 and capi.K_COUNT == 13
    assert len(capi.FA_ROW) == 10 and len(capi.FA_PLANE) == 7 and C.sizeof(capi.FacetParams) == 20


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  ' + "\n  ".join(f"(void){s};" for s in NEW) +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && sizeof(pcp_facet_params) == 20 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["facets_selftest"]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "facets_selftest.cpp")
    exe = str(tmp_path / "facets_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_pipeline_refuses_index_shards():
    from pointcloudprocessor_amd import pipeline

    for call in (lambda p: p.facets(), lambda p: p.ortho_maps_by_facet(0.01)):
        with pytest.raises(ValueError) as e:
            call(pipeline.PointCloudColorizer(None, rank=0, world=2))
        assert "index shard" in str(e.value)
