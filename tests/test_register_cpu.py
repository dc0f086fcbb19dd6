"""CPU suite of the map registration (csrc/pcp_register.hpp through pcp_compare_register_host and pcp_register_solve_host: no
context, no GPU) against the restatement in _register_ref.py ("Map registration", RG1-RG8).  Integers by equality,
floats by bytes; accuracy against the plain fp64 ICP of the same file."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _register_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_default_register_params", "pcp_compare_register_sums", "pcp_register_solve_host", "pcp_compare_register",
       "pcp_compare_base_transform", "pcp_compare_set_base_transform", "pcp_compare_register_host")
QUANTUM = 2.0 ** -20


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@functools.lru_cache(maxsize=None)
def scene(name):
    return {"exact": ref.corner, "resampled": lambda: ref.corner(resampled=True), "wall": ref.wall_alone, "changed": ref.changed}[name]()


@functools.lru_cache(maxsize=None)
def restated(name, **kw):
    c = scene(name)
    return ref.register(c["xyz"], c["normals"], c["base"], **kw)


def host(c, **kw):
    return _capi().compare_register_host(c["xyz"], c["normals"], c["base"], **kw)


def same_run(got, want):
    """None, or the first key of two loop results that differs"""
    for k in ("status", "iterations", "dof", "pairs"):
        if got[k] != want[k]:
            return k
    for k in ("sums",):
        if not np.array_equal(got[k], want[k]):
            return k
    for k in ("T", "log", "rows"):
        if got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes():
            return k
    return None


def bounds_from(plain_err, ell):
    """twice the plain ICP's error plus one offset quantum (in angle: the quantum at the distance ell)"""
    return 2.0 * plain_err[0] + QUANTUM, 2.0 * plain_err[1] + QUANTUM / ell


@pytest.mark.parametrize("name", ("exact", "resampled"))
def test_corner_is_recovered(name):
    """Measured (errors at the pivot in m, rad; bounds = twice the plain ICP's plus 2^-20 m, 2^-20 m / ell):
    exact     ours 6.67e-9, 2.55e-8   plain 3.09e-9, 5.22e-9   bounds 9.60e-7, 1.11e-6   3 iterations, 6000 pairs
    resampled ours 1.8261e-4, 1.1462e-4   plain 1.8262e-4, 1.1435e-4   bounds 3.66e-4, 2.30e-4   4 iterations, rms 1.62 mm"""
    c, want = scene(name), restated(name)
    got = host(c)
    assert same_run(got, want) is None, same_run(got, want)
    assert got["status"] == ref.CONVERGED and got["dof"] == 6
    plain = ref.plain_icp(c["xyz"], c["normals"], c["base"])
    ours, theirs = ref.pose_error(got["T"], c["T_true"], want["pivot"]), ref.pose_error(plain["T"], c["T_true"], want["pivot"])
    bound = bounds_from(theirs, want["ell"])
    print(name, "ours", ours, "plain", theirs, "bounds", bound, "iterations", got["iterations"], "pairs", got["pairs"], "rms", got["rms"])
    assert ours[0] <= bound[0] and ours[1] <= bound[1]
    # the start was 4 mm / 0.2 degrees off
    start = ref.pose_error(np.eye(4), c["T_true"], want["pivot"])
    assert start[0] > 3e-3 and start[1] > 3e-3


def _observable(T, c, axis=2):
    """What one wall with normal +axis shows of the error of T: the shift along the normal at the pivot and the rotation about
    the two in-plane axes"""
    E = np.asarray(T) @ np.linalg.inv(c["T_true"])
    p = np.append(restated("wall")["pivot"], 1.0)
    R = E[:3, :3]
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return abs(((E @ p) - p)[axis]), float(np.hypot(w[(axis + 1) % 3], w[(axis + 2) % 3]))


def test_one_wall_alone():
    """Measured: dof 3, 3 iterations; along the normal 1.038e-5 m (plain 1.037e-5), about the in-plane axes 2.569e-5 rad (plain
    2.566e-5): the partners on a single wall are not the planted ones, for both.  The update's three unobservable components
    are exactly zero."""
    c, want = scene("wall"), restated("wall")
    got = host(c)
    assert same_run(got, want) is None, same_run(got, want)
    assert got["status"] == ref.CONVERGED and got["dof"] == 3 and (got["log"][:, 2] == 3).all()
    plain = ref.plain_icp(c["xyz"], c["normals"], c["base"])
    ours, theirs = _observable(got["T"], c), _observable(plain["T"], c)
    bound = bounds_from(theirs, want["ell"])
    print("wall ours", ours, "plain", theirs, "bounds", bound)
    assert ours[0] <= bound[0] and ours[1] <= bound[1]
    # sliding in the plane and spinning about the normal never move (the 4 x 4 mixes the components: the update shows them)
    capi = _capi()
    sums = capi.compare_register_host(c["xyz"], c["normals"], c["base"], loop=False)["sums"]
    s = capi.register_solve_host(sums, want["ell"])
    assert s["dof"] == 3
    assert s["omega"][2] == 0.0 and s["dt"][0] == 0.0 and s["dt"][1] == 0.0
    assert s["omega"][0] != 0.0 and s["omega"][1] != 0.0 and s["dt"][2] != 0.0


def test_default_cond_tol_separates_the_spectra():
    """The plain ICP's spectra (eigenvalues over the largest) with normals estimated at 0.05 m: corner 1, 0.928, 0.919, 0.199,
    0.195, 0.190; one wall 1, 0.177, 0.163, 2.05e-4, 1.78e-4, 6.8e-5.  The gap is 2.97 decades; the default is its geometric
    mean, sqrt(0.190 * 2.05e-4) = 6.2e-3."""
    import _compare_ref as cref

    lows, highs = [], []
    for walls in ((0, 1, 2), (2,)):
        c = ref.corner(resampled=True, walls=walls)
        sp = ref.plain_icp(c["xyz"], cref.eigh_normals(c["xyz"], 0.05), c["base"])["spectrum"]
        sp = sp / sp[0]
        print("spectrum", walls, sp)
        (lows if len(walls) == 3 else highs).append(sp)
    smallest_seen, largest_unseen = lows[0][5], highs[0][3]
    assert highs[0][2] > smallest_seen * 0.5  # the wall's three observable directions are as strong as the corner's weakest
    assert math.log10(smallest_seen / largest_unseen) >= 2.0
    mean = math.sqrt(smallest_seen * largest_unseen)
    assert 0.8 * mean <= ref.DEFAULT_COND_TOL <= 1.25 * mean
    assert _capi().RG_DEFAULT_COND_TOL == ref.DEFAULT_COND_TOL


def test_wall_with_estimated_normals_keeps_three():
    import _compare_ref as cref

    c = ref.corner(resampled=True, walls=(2,), per_wall=1200)
    normals = cref.eigh_normals(c["xyz"], 0.05)
    got = _capi().compare_register_host(c["xyz"], normals, c["base"])
    want = ref.register(c["xyz"], normals, c["base"])
    assert same_run(got, want) is None, same_run(got, want)
    assert got["dof"] == 3 and got["status"] == ref.CONVERGED


def test_changed_region_is_trimmed():
    """Seed 7, the 5 mm step inside the disc.  max_plane_distance 2 mm: 11 iterations, 4530 of 6000 pairs, error along the
    normal 3.90e-5 m (plain 3.88e-5), about the in-plane axes 1.60e-4 rad (plain 1.60e-4).  At 0.05 (= match_radius) all 6000
    pairs count and the fit is pulled 6.27e-4 m towards the step (not asserted)."""
    c = scene("changed")
    got = host(c, max_plane_distance=0.002)
    want = restated("changed", max_plane_distance=0.002)
    assert same_run(got, want) is None, same_run(got, want)
    assert got["status"] == ref.CONVERGED and got["dof"] == 3
    plain = ref.plain_icp(c["xyz"], c["normals"], c["base"], max_plane_distance=0.002)

    def seen(T):
        E = np.asarray(T) @ np.linalg.inv(c["T_true"])
        p = np.append(want["pivot"], 1.0)
        R = E[:3, :3]
        w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        return abs(((E @ p) - p)[:3] @ c["e_n"]), float(np.hypot(w @ c["e_u"], w @ c["e_v"]))

    ours, theirs = seen(got["T"]), seen(plain["T"])
    bound = bounds_from(theirs, want["ell"])
    pulled = seen(host(c, max_plane_distance=0.05)["T"])
    print("changed ours", ours, "plain", theirs, "bounds", bound, "untrimmed", pulled, "pairs", got["pairs"])
    assert ours[0] <= bound[0] and ours[1] <= bound[1]
    assert got["pairs"] < 5000


def test_the_comparison_after_the_twin_is_as_quiet_as_without_a_shift():
    """The host forms alone, before any device run: the resampled corner compared against its base where it was sampled, 4 mm
    off, and registered.  Measured share of significant among measured points: in place 0.068, off 0.810, registered 0.074."""
    import _compare_ref as cref

    capi = _capi()
    c, want = scene("resampled"), restated("resampled")
    kw = dict(radius=0.03, half_length=0.05, min_points=5)

    def share(base):
        st = capi.compare_host(c["xyz"], c["normals"], base, **kw)["status"]
        return float((st >= 4).sum()) / max(1, int((st >= 3).sum()))

    in_place = share(ref.moved(c["base"], c["T_true"]))
    twin = host(c)  # the CPU twin's own rows, which are also the restatement's
    assert twin["rows"].tobytes() == want["rows"].tobytes()
    off, registered = share(c["base"]), share(twin["rows"])
    print("significant share: in place", in_place, "off", off, "registered", registered)
    assert registered <= in_place + 0.05 < off


BOUNDARIES = ref.boundaries()


@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_boundary(name):
    c = BOUNDARIES[name]
    got = host(c, loop=False, **c["kw"])
    q, t = ref.identity()
    pivot, _ = ref.pivot_of(c["base"])
    want = ref.evaluate(c["xyz"], c["normals"], c["base"], q, t, pivot, ref.params(**c["kw"]))
    assert [int(v) for v in got["sums"]] == want
    assert int(got["sums"][58]) == c["pairs"] and int(got["sums"][59]) == 0
    assert got["rows"].tobytes() == c["base"].tobytes()  # RG1: the identity keeps the bytes, the non-finite rows too


def test_the_tie_rule_shows_in_the_sums():
    def n2_terms(name):
        s = host(BOUNDARIES[name], loop=False)["sums"]
        return [int(s[2 * k]) for k in (15, 18, 20)]  # g3 g3, g4 g4, g5 g5: the squares of the partner's normal

    assert n2_terms("tie_goes_to_the_lowest_index") == [0, 0, 2048 * 2048]
    assert n2_terms("tie_the_other_way") == [0, 2048 * 2048, 0]
    assert n2_terms("duplicated_map_point") == [1229 * 1229, 0, 1638 * 1638]


def test_stride_three():
    c = ref.strided()
    got = host(c, loop=False, **c["kw"])
    q, t = ref.identity()
    pivot, _ = ref.pivot_of(c["base"])
    assert [int(v) for v in got["sums"]] == ref.evaluate(c["xyz"], c["normals"], c["base"], q, t, pivot, ref.params(**c["kw"]))
    every = int(host(c, loop=False)["sums"][58])
    assert 10 <= int(got["sums"][58]) <= 34 < every <= 100


def test_lever_arm_range():
    capi = _capi()
    c = ref.lever_beyond()
    with pytest.raises(capi.PcpError) as e:
        host(c, loop=False)
    assert e.value.code == capi.PCP_ERR_RANGE
    q, t = ref.identity()
    with pytest.raises(ref.RangeError):
        ref.evaluate(c["xyz"], c["normals"], c["base"], q, t, ref.pivot_of(c["base"])[0], ref.params())


def test_fewer_than_min_pairs():
    c = BOUNDARIES["trim_on_the_boundary"]
    got = host(c, min_pairs=3, **c["kw"])
    want = ref.register(c["xyz"], c["normals"], c["base"], min_pairs=3, **c["kw"])
    assert same_run(got, want) is None
    assert got["status"] == ref.TOO_FEW_PAIRS and got["iterations"] == 1 and got["pairs"] == 2
    assert np.array_equal(got["T"], np.eye(4)) and got["rows"].tobytes() == c["base"].tobytes()
    enough = host(c, min_pairs=2, **c["kw"])
    assert enough["status"] != ref.TOO_FEW_PAIRS and enough["log"][0, 2] >= 1


def test_identity_leaves_the_compare_stage_alone():
    import _compare_ref as cref

    capi = _capi()
    c = cref.wall(600, 11)
    base = c["base"].copy()
    base[3] = np.nan
    base[5, 1] = -0.0
    rows = capi.compare_register_host(c["xyz"], c["normals"], base, loop=False)["rows"]
    assert rows.tobytes() == base.tobytes()
    a, b = capi.compare_host(c["xyz"], c["normals"], base, **c["kw"]), capi.compare_host(c["xyz"], c["normals"], rows, **c["kw"])
    assert cref.same_bytes(a, b) is None


def test_a_given_start_is_taken():
    """T_in: the planted motion itself is a fixed point to within the tolerance, and the rows at it are the restatement's"""
    c = scene("exact")
    got = host(c, T_in=c["T_true"])
    assert got["status"] == ref.CONVERGED and got["iterations"] == 1
    assert ref.pose_error(got["T"], c["T_true"], restated("exact")["pivot"])[0] < 1e-6


@pytest.mark.parametrize("rank", (6, 3, 0))
@pytest.mark.parametrize("big", (False, True))
def test_solve_alone(rank, big):
    capi = _capi()
    sums, ell = ref.hand_sums(rank, big=big)
    got = capi.register_solve_host(sums, ell, 1e-6)
    update, eig, dof = ref.solve(sums, ell, 1e-6)
    assert got["dof"] == dof == rank
    assert np.concatenate([got["omega"], got["dt"]]).tobytes() == np.array(update, np.float64).tobytes()
    assert got["eigenvalues"].tobytes() == eig.tobytes()
    assert np.float64(got["rms"]).tobytes() == np.float64(ref.rms_of(sums)).tobytes()
    if rank == 3:
        assert got["omega"][2] == 0 and got["dt"][0] == 0 and got["dt"][1] == 0 and got["dt"][2] != 0
    if rank == 0:
        assert not got["omega"].any() and not got["dt"].any() and got["rms"] == 0
    if big:  # the same geometry scaled: the update does not change beyond rounding, the sums need both halves
        small = capi.register_solve_host(ref.hand_sums(rank)[0], ell, 1e-6)
        assert np.allclose(small["omega"], got["omega"], rtol=1e-6, atol=1e-15) and np.allclose(small["dt"], got["dt"], rtol=1e-6, atol=1e-15)
        assert rank == 0 or abs(int(sums[0]) + (int(sums[1]) << 32)) > 2 ** 63


def test_refusals():
    capi = _capi()
    c = BOUNDARIES["trim_on_the_boundary"]
    below = float(np.nextafter(np.float32(0.005), np.float32(0)))
    for kw in (dict(match_radius=below), dict(match_radius=0.6), dict(match_radius=float("nan")), dict(max_plane_distance=0.0),
               dict(max_plane_distance=0.06), dict(max_plane_distance=float("nan")), dict(sample_stride=0), dict(max_iterations=0),
               dict(max_iterations=1001), dict(min_pairs=0), dict(tolerance=-1e-9), dict(tolerance=float("nan")), dict(cond_tol=0.0),
               dict(cond_tol=1.0)):
        with pytest.raises(capi.PcpError) as e:
            host(c, **kw)
        assert e.value.code == capi.PCP_ERR_INVALID, kw
        assert not ref.params_ok(ref.params(**kw)), kw
    host(c, match_radius=0.005, max_plane_distance=0.005)  # the bounds themselves are taken
    host(c, match_radius=0.5, max_plane_distance=0.5, max_iterations=1)
    big = np.zeros((65537, 3), np.float32)
    small = np.zeros((3, 3), np.float32)
    up = np.tile(np.array([[0, 0, 1]], np.float32), (65537, 1))
    for xyz, nrm, base in ((big, up, small), (small, up[:3], big)):
        with pytest.raises(capi.PcpError) as e:
            capi.compare_register_host(xyz, nrm, base)
        assert e.value.code == capi.PCP_ERR_INVALID
    shear = np.eye(4)
    shear[0, 1] = 1e-3
    with pytest.raises(capi.PcpError) as e:
        host(c, T_in=shear)
    assert e.value.code == capi.PCP_ERR_INVALID
    for ell, tol in ((0.0, 1e-3), (float("nan"), 1e-3), (1.0, 0.0), (1.0, 1.0)):
        with pytest.raises(capi.PcpError) as e:
            capi.register_solve_host(np.zeros(60, np.int64), ell, tol)
        assert e.value.code == capi.PCP_ERR_INVALID
    lib = capi.load()
    prm = capi.register_params()
    assert lib.pcp_compare_register(None, capi.C.byref(prm), None, None, None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_compare_register_sums(None, capi.C.byref(prm), None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_compare_base_transform(None, None, None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_compare_set_base_transform(None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_compare_register_host(None, capi.C.c_int64(0), None, None, capi.C.c_int64(0), None, None, capi.C.c_int32(0), None,
                                         None, None, None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_register_solve_host(None, capi.C.c_double(1.0), capi.C.c_double(1e-3), None, None, None) == capi.PCP_ERR_INVALID


def test_empty_clouds():
    capi = _capi()
    none = np.zeros((0, 3), np.float32)
    c = BOUNDARIES["trim_on_the_boundary"]
    for xyz, nrm, base in ((none, none, c["base"]), (c["xyz"], c["normals"], none)):
        got = capi.compare_register_host(xyz, nrm, base)
        assert got["status"] == ref.TOO_FEW_PAIRS and got["pairs"] == 0 and not got["sums"].any() and np.array_equal(got["T"], np.eye(4))


def test_default_params():
    capi = _capi()
    lib = capi.load()
    lib.pcp_default_register_params.restype = None
    prm = capi.RegisterParams()
    prm.min_pairs = -7
    lib.pcp_default_register_params(capi.C.byref(prm))
    assert (prm.match_radius, prm.max_plane_distance, prm.sample_stride, prm.max_iterations, prm.min_pairs, prm.tolerance, prm.cond_tol) == (
        np.float32(0.05), np.float32(0.02), 1, 20, 100, 1e-5, ref.DEFAULT_COND_TOL)
    assert capi.C.sizeof(capi.RegisterParams) == 40
    mine = capi.register_params()
    assert bytes(mine) == bytes(prm)


def test_header_constants():
    text = open(os.path.join(ROOT, "pointcloudprocessor_amd", "csrc", "pcp_register.hpp")).read()
    for line in ("kTerms = 30", "kLeverScale = 256.0", "kMaxLever = int64_t(1) << 18", "kSweeps = 12", "kDefaultCondTol = 6.2e-3"):
        assert line in text, line
    assert ref.LEVER == 256.0 and ref.MAX_LEVER == 2 ** 18 and ref.SWEEPS == 12 and len(_capi().RG_TERMS) == 30


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    for m in ("compare_register_sums", "compare_register", "compare_base_transform", "compare_set_base_transform"):
        assert callable(getattr(capi.Context, m)), m
    assert callable(capi.compare_register_host) and callable(capi.register_solve_host)
    assert lib.pcp_abi_version() == 6 and capi.K_COUNT == 13


def test_header_with_the_new_declarations_is_plain_c(tmp_path):
    src = tmp_path / "abi.c"
    calls = "\n".join(f"  (void){s};" for s in NEW)
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n' + calls +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && sizeof(pcp_register_params) == 40 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["register_selftest"]
    out = subprocess.run([exe, "600"], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "register_selftest.cpp")
    exe = str(tmp_path / "register_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe, "300"], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr
