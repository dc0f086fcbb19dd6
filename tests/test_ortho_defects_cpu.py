"""CPU suite of the surface defects on ortho maps (csrc/pcp_ortho_defects.hpp through pcp_ortho_defects_host: no context, no
GPU) against the restatement in _ortho_defects_ref.py, bit for bit: the three layers, the eight counts and the table on every
raster the device suite uses; the refusals and their messages, the ABI, the stand-alone self-test plain and under the host
sanitizers, and the cap scene against its analytic values.

The cap scene (SD rules, "measured"): lattice of half the gsd, seed 7, t = 2 mm, W = 0.  Restated on this seed:
gsd 4 mm: area off by 0.15 / 0.16 of the band, volume by 7.0 % / 7.3 %; gsd 2 mm: 0.18 / 0.16 and 3.7 % / 3.6 % (hollow /
bulge).  W = 40 at 4 mm: greatest depth 11.56 / 11.50 mm without refine, 11.96 / 11.98 mm with it, of 12 mm."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _ortho_defects_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_ortho_defects", "pcp_ortho_defects_fetch", "pcp_ortho_defects_table", "pcp_ortho_defects_host")
CASES = ref.cases()


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.mark.parametrize("name,spec,kw", CASES, ids=[c[0] for c in CASES])
def test_host_twin_equals_the_restatement(name, spec, kw):
    capi = _capi()
    depth, status = ref.raster(spec)
    want = ref.defects(depth, status, **kw)
    got = capi.ortho_defects_host(depth, status, **kw)
    print(name, dict(zip(ref.OUT, want["out"])))
    assert ref.same(got, want) is None, ref.same(got, want)


def test_the_cases_hold_what_they_are_for():
    """The preconditions of the shared cases, on the restatement's own counts: a check of the fixtures, not of the feature (it
    needs no library and would pass without the stage); it keeps the cases from going blunt under a later edit."""
    w = {c[0]: ref.defects(*ref.raster(c[1]), **c[2]) for c in CASES}
    big = w["random-242x202-W7-r1"]["out"]
    assert big[0] >= 100 and big[1] >= 100 and big[2] >= 500 and big[3] >= 500 and big[5] == 6 and big[6] >= 10
    assert w["random-257x1-W1-r0"]["out"][4] >= 5  # unsupported pixels
    assert w["random-70x60-W5-support20-bulges"]["out"][2] == 0 and w["random-70x60-W5-support20-bulges"]["out"][6] >= 50
    assert (w["random-70x60-W5-support20-bulges"]["rows"][:, ref.R_FIRST_PASS] > 0).any()
    assert list(w["diagonal"]["out"][:3]) == [1, 0, 257] and list(w["spiral"]["out"][:2]) == [1, 0] and w["spiral"]["out"][2] > 8000
    tc = w["tile-corners"]
    assert list(tc["out"][:4]) == [4, 0, 44, 2] and sorted(tc["rows"][:, ref.R_PIXELS]) == [2, 2, 2, 40]
    cb = w["checkerboard"]
    assert list(cb["out"][:2]) == [2, 0] and sorted(cb["rows"][:, ref.R_CLASS]) == [1, 2] and list(cb["rows"][:, ref.R_FIRST]) == [0, 1]
    rv = w["reversed-sizes"]["rows"]
    assert len(rv) == 2 and rv[0, ref.R_PIXELS] < rv[1, ref.R_PIXELS] and rv[0, ref.R_FIRST] < rv[1, ref.R_FIRST]
    mp = w["min-pixels"]
    assert list(mp["out"][:2]) == [1, 1] and mp["rows"][0, ref.R_PIXELS] == 5 and (mp["cls"] == 1).sum() == 4 and (mp["region"][mp["cls"] == 1] == 0).all()
    em = w["equal-maxima"]["rows"][0]
    assert em[ref.R_MAX] == round(0.02 * ref.Q) and em[ref.R_MAX_PIXEL] == 9 * 30 + 8
    eh = w["edge-and-hole"]["rows"]
    assert eh[0, ref.R_OPEN] == 8 and eh[1, ref.R_OPEN] == 14 and eh[1, ref.R_MEASURED] == eh[1, ref.R_PIXELS] - 1
    assert list(w["no-defects"]["out"][:4]) == [0, 0, 0, 0] and w["no-defects"]["out"][7] == 20 * 33


def test_nothing_but_empty_pixels_and_refused_depths():
    capi = _capi()
    depth = np.full((5, 9), np.nan, np.float32)
    depth[2, 3:6] = (600.0, -np.inf, 0.01)
    status = np.zeros((5, 9), np.uint8)
    status[2, 3:5] = (1, 2)
    for W in (0, 3):
        got = capi.ortho_defects_host(depth, status, window=W)
        assert ref.same(got, ref.defects(depth, status, window=W)) is None
        assert list(got["out"]) == [0, 0, 0, 0, 0, 2, 0, 0] and got["rows"].shape == (0, 16)


def test_refusals_name_the_field():
    capi = _capi()
    depth, status = ref.flat(4, 5)
    assert capi.ortho_defects_host(depth, status, threshold=2.0 ** -20, window=1024, refine=True)["out"][7] == 20
    assert capi.ortho_defects_host(depth, status, threshold=1.0, min_support=0)["out"][7] == 20  # (min_support is not read at W = 0)
    bad = ((dict(threshold=2.0 ** -21), "threshold"), (dict(threshold=1.001), "threshold"), (dict(threshold=float("nan")), "threshold"),
           (dict(threshold=float("inf")), "threshold"), (dict(threshold=-0.002), "threshold"), (dict(window=-1), "window_px"),
           (dict(window=1025), "window_px"), (dict(window=3, refine=2), "refine"), (dict(window=0, refine=1), "refine"),
           (dict(window=3, min_support=0), "min_support"), (dict(min_pixels=0), "min_pixels"), (dict(classes=0), "classes"),
           (dict(classes=4), "classes"))
    for kw, word in bad:
        with pytest.raises(capi.PcpError) as e:
            capi.ortho_defects_host(depth, status, **kw)
        assert e.value.code == capi.PCP_ERR_INVALID and word in str(e.value) and "pcp_ortho_defects_host" in str(e.value), (kw, str(e.value))
    L = capi.load()
    p = capi.ortho_defect_params()
    out = np.zeros(8, np.int64)
    n = C.c_int64(7)
    args = (capi._ptr(depth), capi._ptr(status), C.byref(p), capi._ptr(out), None, None, None, None, C.c_int64(0), C.byref(n))
    assert L.pcp_ortho_defects_host(C.c_int32(5), C.c_int32(4), *args) == capi.PCP_OK and n.value == 0
    for w, h in ((0, 4), (5, 0), (16385, 1), (8193, 8193)):
        assert L.pcp_ortho_defects_host(C.c_int32(w), C.c_int32(h), *args) == capi.PCP_ERR_INVALID
        assert "width" in L.pcp_last_error(None).decode()
    assert L.pcp_ortho_defects_host(C.c_int32(5), C.c_int32(4), None, capi._ptr(status), C.byref(p), capi._ptr(out), None, None, None, None,
                                    C.c_int64(0), None) == capi.PCP_ERR_INVALID
    assert L.pcp_ortho_defects_host(C.c_int32(5), C.c_int32(4), capi._ptr(depth), capi._ptr(status), None, capi._ptr(out), None, None, None,
                                    None, C.c_int64(0), None) == capi.PCP_ERR_INVALID


def test_the_table_is_cut_at_max_rows():
    capi = _capi()
    L = capi.load()
    depth, status = ref.raster(("random", 60, 70))
    want = ref.defects(depth, status)
    assert len(want["rows"]) > 3
    p = capi.ortho_defect_params()
    out = np.zeros(8, np.int64)
    rows = np.full((4, 16), -1, np.int64)
    n = C.c_int64()
    assert L.pcp_ortho_defects_host(C.c_int32(70), C.c_int32(60), capi._ptr(depth), capi._ptr(status), C.byref(p), capi._ptr(out), None, None,
                                    None, capi._ptr(rows), C.c_int64(3), C.byref(n)) == capi.PCP_OK
    assert n.value == len(want["rows"]) and np.array_equal(rows[:3], want["rows"][:3]) and (rows[3] == -1).all()


@pytest.fixture(scope="module")
def cap_maps():
    """the cap scene's maps at both gsd by the host form of the ortho maps: computed once, left unchanged"""
    capi = _capi()
    out = {}
    for gsd in (0.004, 0.002):
        xyz = ref.cap_scene(gsd)
        m = capi.ortho_host(ref.cap_frame(gsd), xyz, np.zeros((len(xyz), 3), np.uint8))
        assert m["occupied"] == m["depth"].size  # no fill: every pixel measured
        for a in (m["depth"], m["status"]):
            a.setflags(write=False)
        out[gsd] = m
    return out


@pytest.mark.parametrize("gsd", [0.004, 0.002])
def test_cap_scene_meets_its_analytic_values(cap_maps, gsd):
    capi = _capi()
    m = cap_maps[gsd]
    got = capi.ortho_defects_host(m["depth"], m["status"], threshold=ref.CAP_T, window=0)
    assert ref.same(got, ref.defects(m["depth"], m["status"], threshold=ref.CAP_T, window=0)) is None
    band, volume_bound, depth_bound = ref.cap_bounds(gsd)
    measures = ref.cap_measures(got["rows"], gsd)
    assert [k for k, _, _, _ in measures] == [1, 2]  # the hollow lies left of the bulge
    for k, area, volume, depth in measures:
        print(f"gsd {gsd} class {k}: area off by {(area - ref.CAP_AREA) / band:+.3f} of the band, volume by "
              f"{(volume - ref.CAP_VOLUME) / ref.CAP_VOLUME:+.4f} (bound {volume_bound}), greatest depth by {depth - ref.CAP_H:+.2e} m (bound {depth_bound:.2e})")
        assert abs(area - ref.CAP_AREA) <= band
        assert abs(volume - ref.CAP_VOLUME) <= volume_bound * ref.CAP_VOLUME
        assert abs(depth - ref.CAP_H) <= depth_bound
    for (cx, cy), row in zip(ref.CAP_CENTRES, got["rows"]):  # the centroids, within a pixel
        assert abs((row[ref.R_SUM_COL] / row[ref.R_PIXELS] + 0.5) * gsd - cx) <= gsd
        assert abs((row[ref.R_SUM_ROW] / row[ref.R_PIXELS] + 0.5) * gsd - cy) <= gsd
        assert row[ref.R_OPEN] == 0 and row[ref.R_MEASURED] == row[ref.R_PIXELS]


def test_refine_reads_the_cap_deeper(cap_maps):
    capi = _capi()
    m = cap_maps[0.004]
    depth = {}
    for refine in (False, True):
        got = capi.ortho_defects_host(m["depth"], m["status"], threshold=ref.CAP_T, window=40, refine=refine)
        assert ref.same(got, ref.defects(m["depth"], m["status"], threshold=ref.CAP_T, window=40, refine=refine)) is None
        assert sorted(got["rows"][:, ref.R_CLASS]) == [1, 2]
        depth[refine] = {int(r[ref.R_CLASS]): r[ref.R_MAX] / ref.Q for r in got["rows"]}
    print("greatest depth, W = 40:", depth)
    for k in (1, 2):
        assert abs(depth[True][k] - ref.CAP_H) < abs(depth[False][k] - ref.CAP_H)


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    assert callable(capi.Context.ortho_defects) and callable(capi.Context.ortho_defects_fetch) and callable(capi.Context.ortho_defects_table)
    assert callable(capi.ortho_defects_host)
    assert lib.pcp_abi_version() == 6 and capi.K_COUNT == 13
    assert C.sizeof(capi.OrthoDefectParams) == 24 and len(capi.DEFECT_OUT) == 8 and len(capi.DEFECT_ROW) == 16


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  ' + "\n  ".join(f"(void){s};" for s in NEW) +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && sizeof(pcp_ortho_defect_params) == 24 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["ortho_defects_selftest"]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "ortho_defects_selftest.cpp")
    exe = str(tmp_path / "ortho_defects_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr
