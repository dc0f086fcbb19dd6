"""CPU suite of the geometry maps (csrc/pcp_normals.hpp through pcp_normals_moments_host: no context, no GPU) against the
restatement in _geometry_ref.py.  Every comparison of moments is exact equality of all ten integers."""
import os
import subprocess

import numpy as np
import pytest

import _geometry_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_estimate_normals", "pcp_normals_fetch", "pcp_normals_moments_host", "pcp_frame_geometry")
# radius -> (fewest neighbours, most neighbours, points with fewer than 3) on synth.make_cloud(20000)
RADII = {0.3: (2, 44, 5), 0.5: (13, 138, 0), 1.0: (91, 505, 0)}


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def cloud():
    from pointcloudprocessor_amd import synth

    x, y, z, _ = synth.make_cloud(20000)
    return np.stack([x, y, z], axis=1)


@pytest.fixture(scope="module")
def host_moments(cloud):
    """radius -> moments of the plain cloud by the library's CPU form, computed once."""
    capi = _capi()
    return {r: capi.normals_moments_host(r, cloud) for r in RADII}


@pytest.mark.parametrize("radius", sorted(RADII))
def test_host_form_equals_the_restatement(cloud, host_moments, radius):
    got = host_moments[radius]
    want = ref.moments(radius, cloud)
    assert got.dtype == np.int64 and got.shape == (len(cloud), 10)
    assert np.array_equal(got, want)
    lo, hi, few = RADII[radius]
    assert (int(got[:, 0].min()), int(got[:, 0].max()), int((got[:, 0] < 3).sum())) == (lo, hi, few)


@pytest.mark.parametrize("radius", sorted(RADII))
def test_duplicates_and_non_finite_points(cloud, radius):
    xyz = ref.dirty_cloud(cloud)
    got = _capi().normals_moments_host(radius, xyz)
    assert np.array_equal(got, ref.moments(radius, xyz))
    bad = ~np.isfinite(xyz).all(axis=1)
    assert bad.sum() == 2 and not got[bad].any()  # GN1: not a query
    assert (got[~bad, 0] >= 1).all()  # a finite point is its own neighbour
    assert (got[len(cloud):][~bad[len(cloud):], 0] >= 2).all()  # ... and a duplicate's neighbour


def test_permuting_the_input_permutes_the_rows(cloud, host_moments):
    p = np.random.default_rng(5).permutation(len(cloud))
    again = _capi().normals_moments_host(0.5, cloud[p])
    assert np.array_equal(again, host_moments[0.5][p])


def test_refusals():
    capi = _capi()
    xyz = np.zeros((4, 3), np.float32)
    for r in (float("nan"), 0.0, 0.0049, 1.0001, -0.1, float("inf")):
        with pytest.raises(capi.PcpError) as e:
            capi.normals_moments_host(r, xyz)
        assert e.value.code == capi.PCP_ERR_INVALID, r
    with pytest.raises(capi.PcpError) as e:
        capi.normals_moments_host(0.1, np.zeros((65537, 3), np.float32))
    assert e.value.code == capi.PCP_ERR_INVALID
    assert capi.normals_moments_host(0.1, np.zeros((0, 3), np.float32)).shape == (0, 10)
    got = capi.normals_moments_host(0.005, xyz)  # four copies of the origin
    assert (got[:, 0] == 4).all() and not got[:, 1:].any()
    lib = capi.load()
    assert lib.pcp_estimate_normals(None, capi.C.c_float(0.1), None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_normals_fetch(None, None, None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_frame_geometry(None, capi.C.c_int32(0), None, None, None, None, None) == capi.PCP_ERR_INVALID


def test_threshold_is_the_largest_float_not_above_the_square():
    for r in (0.005, 0.03, 0.1, 0.3, 0.5, 1.0):
        t = ref.threshold(r)
        r2 = float(np.float32(r)) ** 2
        assert float(t) <= r2 < float(np.nextafter(t, np.float32(2.0)))


def test_header_constants():
    text = open(os.path.join(ROOT, "pointcloudprocessor_amd", "csrc", "pcp_normals.hpp")).read()
    for line in ("kQuantaPerMetre = 1048576.0f", "kMaxQuantum = (1 << 20) + 1", "kMaxNeighbours = int64_t(1) << 22", "kMinNeighbours = 3",
                 "kMomentWords = 10"):
        assert line in text, line
    assert ref.Q == 2.0 ** 20


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    for m in ("estimate_normals", "normals_fetch", "frame_geometry"):
        assert callable(getattr(capi.Context, m)), m
    assert callable(capi.normals_moments_host) and lib.pcp_abi_version() == 6 and capi.K_COUNT == 13


def test_header_with_the_new_declarations_is_plain_c(tmp_path):
    src = tmp_path / "abi.c"
    calls = "\n".join(f"  (void){s};" for s in NEW)
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n' + calls + "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["normals_selftest"]
    out = subprocess.run([exe, "600"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "normals_selftest.cpp")
    exe = str(tmp_path / "normals_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe, "300"], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_pipeline_refuses_index_shards():
    from pointcloudprocessor_amd import pipeline

    with pytest.raises(ValueError) as e:
        pipeline.PointCloudColorizer(None, rank=0, world=2).geometry_maps(0)
    assert "index shard" in str(e.value) and "not built" in str(e.value)
