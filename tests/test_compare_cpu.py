"""CPU suite of the map comparison (csrc/pcp_compare.hpp through pcp_compare_host: no context, no GPU) against the restatement
in _compare_ref.py ("Map comparison", MC1-MC6).  Integers, status and stats by equality, distance and lod by bytes."""
import os
import subprocess

import numpy as np
import pytest

import _compare_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_default_compare_params", "pcp_compare_set_base", "pcp_compare", "pcp_compare_fetch", "pcp_compare_host", "pcp_compare_end")


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


CASES, case_and_ref = ref.CASES, ref.case_and_ref


def host(c, **over):
    kw = dict(c["kw"])
    kw.update(over)
    return _capi().compare_host(c["xyz"], c["normals"], c["base"], **kw)


@pytest.mark.parametrize("name", CASES)
def test_host_form_equals_the_restatement(name):
    c, want = case_and_ref(name)
    got = host(c)
    assert ref.same_bytes(got, want) is None, ref.same_bytes(got, want)
    assert np.array_equal(got["stats"], ref.stats_of(got["status"], got["sums"]))
    assert not got["distance"][got["status"] < 3].any() and not got["lod"][got["status"] < 3].any()
    zero = got["status"] == 0
    assert not got["sums"][zero].any() and not got["direction"][zero].any()
    assert (got["sums"][~zero, 0] >= 1).all()  # a core point is its own candidate in epoch A


def test_bump_is_found():
    """Seed 7: 99.92 % of the points are measured; inside the disc shrunk by 0.04 all 446 points are status 4, the mean distance
    is +5.03 mm and the worst error against 5 mm is 1.44 mm; outside the disc grown by 0.04 and 0.05 from the border 5.5 % of
    3818 points are flagged against a nominal 5 %."""
    c, got = case_and_ref("bump")
    uv = c["uv"]
    rad = np.hypot(uv[:, 0] - 0.5, uv[:, 1] - 0.5)
    inside = rad < 0.2 - 0.04
    outside = (rad > 0.2 + 0.04) & (uv.min(axis=1) > 0.05) & (uv.max(axis=1) < 0.95)
    print("measured", (got["status"] >= 3).mean(), "inside", inside.sum(), got["distance"][inside].mean(),
          np.abs(got["distance"][inside] - 0.005).max(), "outside", outside.sum(), (got["status"][outside] >= 4).mean())
    assert inside.sum() > 300 and outside.sum() > 3000
    assert (got["status"][inside] == 4).all()
    assert (np.abs(got["distance"][inside].astype(np.float64) - 0.005) <= 0.0015).all()
    assert (got["status"][outside] >= 4).mean() <= 0.10
    assert (got["status"] >= 3).mean() >= 0.99


def test_permuting_both_clouds_permutes_the_rows():
    c = ref.wall(1500, 11)
    plain = host(c)
    shuffled, pa = ref.permute(c)
    again = host(shuffled)
    for k in ("distance", "lod", "status", "sums", "direction"):
        assert again[k].tobytes() == plain[k][pa].tobytes(), k
    assert np.array_equal(again["stats"], plain["stats"])
    assert ref.same_bytes(again, ref.compare(shuffled["xyz"], shuffled["normals"], shuffled["base"], **shuffled["kw"])) is None


def _assert_flipped(a, b):
    assert np.array_equal(a["sums"][:, [0, 2, 3, 4, 6, 7]], b["sums"][:, [0, 2, 3, 4, 6, 7]])
    assert np.array_equal(a["sums"][:, [1, 5]], -b["sums"][:, [1, 5]])
    assert np.array_equal(a["direction"], -b["direction"])
    assert a["distance"].tobytes() == (-b["distance"] + np.float32(0)).tobytes() or np.array_equal(a["distance"], -b["distance"])
    assert np.array_equal(a["lod"], b["lod"])
    swap = np.array([0, 1, 2, 3, 5, 4], np.uint8)
    assert np.array_equal(a["status"], swap[b["status"]])
    assert (a["status"] == 4).sum() > 0 and (a["status"] == 5).sum() > 0


def test_flip():
    c = ref.wall(1500, 11)
    front = host(c)
    viewer = np.array(c["kw"]["orient"], np.float64)
    behind = viewer - 2 * 2.0 * ref.E_N  # the same distance on the other side of the wall
    back = host(c, orient=tuple(behind))
    _assert_flipped(back, front)
    along = host(c, orient_mode=2, orient=tuple(ref.E_N))
    against = host(c, orient_mode=2, orient=tuple(-ref.E_N))
    _assert_flipped(against, along)
    assert ref.same_bytes(along, front) is None  # (every normal of the wall is within a right angle of its own axis)
    # mode 0 follows the given sign
    given = host(c, orient_mode=0)
    negated = _capi().compare_host(c["xyz"], -c["normals"], c["base"], **dict(c["kw"], orient_mode=0))
    _assert_flipped(negated, given)
    assert np.array_equal(given["direction"], np.rint(c["normals"] * np.float32(2048)).astype(np.int32))
    for res, kw in ((back, dict(orient=tuple(behind))), (against, dict(orient_mode=2, orient=tuple(-ref.E_N))), (given, dict(orient_mode=0))):
        assert ref.same_bytes(res, ref.compare(c["xyz"], c["normals"], c["base"], **dict(c["kw"], **kw))) is None


def test_boundary():
    c, want = case_and_ref("boundary")
    rc2, L2 = ref.squares(c["kw"]["radius"], c["kw"]["half_length"])
    assert 52428 ** 2 <= L2 < 52429 ** 2 and rc2 == 32765 ** 2 == 19659 ** 2 + 26212 ** 2
    got = host(c)
    assert got["sums"][0, 0] == 1 and got["sums"][0, 4] == sum(c["taken"]) == 5
    # row by row: a base of that one row alone
    for row, taken in zip(c["base"], c["taken"]):
        one = _capi().compare_host(c["xyz"], c["normals"], row[None, :], **c["kw"])
        assert one["sums"][0, 4] == (1 if taken else 0), (row, taken)
    assert got["status"][1] == 1 and got["sums"][1, 4] == 0  # the far map point sees none of them


def test_sphere_comes_before_the_cylinder():
    c, want = case_and_ref("sphere_corner")
    got = host(c)
    d = (c["base"][0] - c["xyz"][0]).astype(np.float32)
    q = np.rint(d * np.float32(ref.Q)).astype(np.int64)
    rc2, L2 = ref.squares(c["kw"]["radius"], c["kw"]["half_length"])
    assert q[2] ** 2 <= L2 and q[0] ** 2 + q[1] ** 2 <= rc2  # inside the integer cylinder ...
    d2 = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    assert d2 > ref.threshold(ref.search_radius(c["kw"]["radius"], c["kw"]["half_length"]))  # ... and outside the sphere
    assert got["sums"][0, 4] == 2  # the corner itself and the near row


def test_tilted_normals_are_rounded_not_truncated():
    c, want = case_and_ref("tilted")
    got = host(c)
    assert got["direction"][0].tolist() == [1229, 0, 1638] and got["direction"][1].tolist() == [-1229, 1638, 0]
    assert got["direction"][2].tolist() == [0, 0, 2048] and got["direction"][3].tolist() == [2, 0, 2048]
    assert got["status"][4] == 0 and not got["direction"][4].any()


def test_min_points():
    c, want = case_and_ref("min_points_case")
    got = host(c)
    st = np.array(c["want"])
    assert np.array_equal(got["status"][st != 3], st[st != 3]) and (got["status"][st == 3] >= 3).all()
    assert np.array_equal(got["sums"][:, 0], [4] * 4 + [5] * 5 + [5] * 5 + [4] * 4)
    assert np.array_equal(got["sums"][:, 4], [5] * 4 + [5] * 5 + [4] * 5 + [4] * 4)
    assert (host(c, min_points=4)["status"] >= 3).all() and (host(c, min_points=6)["status"] == 1).all()


def test_no_counterpart():
    c = ref.wall(600, 13)
    away = host(dict(c, base=c["base"] + np.float32(1.0)))
    empty = host(dict(c, base=np.zeros((0, 3), np.float32)))
    core = ref.directions(c["xyz"], c["normals"], 1, c["kw"]["orient"])[0]
    for got in (away, empty):
        assert np.array_equal(got["status"], core.astype(np.uint8)) and not got["distance"].any() and not got["lod"].any()
        assert got["stats"][4] == core.sum() == got["stats"][0] and not got["sums"][:, 4:].any()
    assert ref.same_bytes(empty, ref.compare(c["xyz"], c["normals"], np.zeros((0, 3), np.float32), **c["kw"])) is None


def test_non_finite_rows_and_invalid_normals_are_status_0():
    c, want = case_and_ref("non_finite")
    got = host(c)
    assert not got["status"][c["bad"]].any() and (got["status"] == 0).sum() >= len(c["bad"])
    clean = np.isfinite(c["base"]).all(axis=1)
    assert ref.same_bytes(_capi().compare_host(c["xyz"], c["normals"], c["base"][clean], **c["kw"]), got) is None


def test_duplicates_count_once_each():
    c, want = case_and_ref("duplicates")
    got = host(c)
    spot = got["sums"][c["spot"]]
    assert (spot[:, 0] == 6).all() and (spot[:, 4] == 6).all() and not spot[:, 1].any()
    assert (got["lod"][c["spot"]] == 0).all() and (got["status"][c["spot"]] == 4).all()
    assert np.allclose(got["distance"][c["spot"]], 0.002, atol=2e-6)
    assert (got["sums"][:60, 0] >= 3).all()  # a point, its two copies


def test_wide_products_stay_inside_int64():
    c, want = case_and_ref("wide")
    assert ref.search_radius(c["kw"]["radius"], c["kw"]["half_length"]) == np.float32(0.5)
    worst = ref.products_fit(c["xyz"], c["normals"], c["base"], c["kw"]["radius"], c["kw"]["half_length"])
    print(worst)
    assert worst["h"] < 2 ** 31 and worst["hh"] < 2 ** 62 and worst["neg"] >= 0
    assert max(worst["Q2N2"], worst["rc2N2"], worst["L2N2"]) < 2 ** 62
    assert worst["Q2N2"] > 2 ** 59  # (the offsets do reach the rim)
    assert want["stats"][6] > 50


def test_crowded_cell():
    c, want = case_and_ref("crowded")
    knot = c["xyz"][:70]
    assert np.ptp(knot, axis=0).max() <= 0.0021
    s = float(ref.search_radius(0.03, 0.05))
    for pts in (c["xyz"], c["base"]):
        assert (np.linalg.norm(pts.astype(np.float64) - knot[0].astype(np.float64), axis=1) < s).sum() >= 600
    assert (want["status"][:600] == 5).all()


def test_refusals():
    capi = _capi()
    c = ref.min_points_case()
    below = float(np.nextafter(np.float32(0.005), np.float32(0)))
    for kw in (dict(radius=below), dict(half_length=below), dict(radius=0.3, half_length=0.4), dict(radius=float("nan")),
               dict(half_length=float("inf")), dict(min_points=1), dict(reg_error=-1e-9), dict(reg_error=float("nan")),
               dict(orient_mode=3), dict(orient_mode=-1), dict(orient_mode=1, orient=(float("nan"), 0, 0))):
        with pytest.raises(capi.PcpError) as e:
            host(c, **kw)
        assert e.value.code == capi.PCP_ERR_INVALID, kw
        if "orient" not in kw:  # the restatement draws the same line
            full = dict(dict(radius=0.03, half_length=0.05), **kw)
            assert not ref.params_ok(full.pop("radius"), full.pop("half_length"), **full), kw
    host(c, radius=0.005, half_length=0.005, min_points=2)  # the bounds themselves are taken
    big = np.zeros((65537, 3), np.float32)
    small = np.zeros((3, 3), np.float32)
    up = np.tile(np.array([[0, 0, 1]], np.float32), (65537, 1))
    for xyz, nrm, base in ((big, up, small), (small, up[:3], big)):
        with pytest.raises(capi.PcpError) as e:
            capi.compare_host(xyz, nrm, base)
        assert e.value.code == capi.PCP_ERR_INVALID
    assert capi.compare_host(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), small)["status"].shape == (0,)
    lib = capi.load()
    prm = capi.compare_params()
    assert lib.pcp_compare(None, capi.C.byref(prm), None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_compare_set_base(None, None, capi.C.c_int64(0), capi.C.c_int64(12)) == capi.PCP_ERR_INVALID
    assert lib.pcp_compare_fetch(None, None, None, None, None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_compare_end(None) == capi.PCP_ERR_INVALID
    assert lib.pcp_compare_host(None, capi.C.c_int64(0), None, None, capi.C.c_int64(0), None, None, None, None, None, None, None) == capi.PCP_ERR_INVALID


def test_default_params():
    capi = _capi()
    lib = capi.load()
    lib.pcp_default_compare_params.restype = None
    prm = capi.CompareParams()
    prm.min_points = -7
    lib.pcp_default_compare_params(capi.C.byref(prm))
    assert (prm.cyl_radius, prm.cyl_half_length, prm.reg_error, prm.min_points, prm.orient_mode, list(prm.orient)) == (
        np.float32(0.03), np.float32(0.05), 0.0, 5, 0, [0.0, 0.0, 0.0])
    assert capi.C.sizeof(capi.CompareParams) == 32


def test_header_constants():
    text = open(os.path.join(ROOT, "pointcloudprocessor_amd", "csrc", "pcp_compare.hpp")).read()
    for line in ("kNormalScale = 2048.0f", "kMaxCandidates = int64_t(1) << 22", "kSumWords = 8", "kMinExtent = 0.005f, kMaxSearch = 0.5f"):
        assert line in text, line
    assert ref.NQ == 2048.0 and ref.Q == 2.0 ** 20


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    for m in ("compare_set_base", "compare", "compare_fetch", "compare_end"):
        assert callable(getattr(capi.Context, m)), m
    assert callable(capi.compare_host) and lib.pcp_abi_version() == 6 and capi.K_COUNT == 13


def test_header_with_the_new_declarations_is_plain_c(tmp_path):
    src = tmp_path / "abi.c"
    calls = "\n".join(f"  (void){s};" for s in NEW)
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n' + calls +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && sizeof(pcp_compare_params) == 32 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["compare_selftest"]
    out = subprocess.run([exe, "600"], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "compare_selftest.cpp")
    exe = str(tmp_path / "compare_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe, "300"], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr
