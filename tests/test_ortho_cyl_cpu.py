"""CPU suite of the cylindrical facets (csrc/pcp_ortho_cyl.hpp through pcp_cyl_angle_host, pcp_ortho_cyl_host and
pcp_cyl_fit_host: no context, no GPU) against the restatement in _ortho_cyl_ref.py: the angle and the map by exact equality,
the fit within 1e-9 relative (directions 1e-6) and against the scenes' ground truth; the refusals, the ABI and the stand-alone
self-test plain and under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _ortho_cyl_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_ortho_begin_cyl", "pcp_ortho_cyl_host", "pcp_cyl_angle_host", "pcp_cyl_fit_host")
SIGMA = 0.002  # radial noise of the scenes, metres
#          N      R    H  arc          ball
FAMILIES = ((20000, 1.0, 3.0, np.pi, 0.1), (20000, 0.5, 3.0, 2 * np.pi, 0.1), (20000, 3.0, 4.0, np.pi / 2, 0.15), (6000, 0.4, 2.0, 2 * np.pi, 0.08))
GSD = 0.01


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def fitted():
    """the twelve scenes with PCA normals over the ball and the restatement's fit of each: computed once, left unchanged"""
    out = {}
    for fam, (N, R, H, arc, ball) in enumerate(FAMILIES):
        for seed in (1, 2, 3):
            sc = ref.cylinder_scene(N, R, H, arc, SIGMA, seed)
            normal = ref.pca_normals(sc["xyz"], ball)
            frame, stats = ref.fit(sc["xyz"], normal, GSD)
            for a in (sc["xyz"], normal):
                a.setflags(write=False)
            out[(fam, seed)] = dict(scene=sc, normal=normal, frame=frame, stats=stats)
    return out


def _wrap_error(theta, s, t):
    d = np.abs(theta - np.mod(np.arctan2(t, s), 2 * np.pi))
    return np.minimum(d, 2 * np.pi - d)


def test_angle_equals_the_restatement_and_atan2():
    capi = _capi()
    rng = np.random.default_rng(11)
    s = np.concatenate([rng.normal(size=340000) * k for k in (1e-3, 1.0, 1e3)])
    t = np.concatenate([rng.normal(size=340000) * k for k in (1e-3, 1.0, 1e3)])
    assert len(s) >= 10 ** 6
    got = capi.cyl_angle_host(s, t)
    assert got.tobytes() == ref.angle(s, t).tobytes()
    err = _wrap_error(got, s, t)
    print("random pairs: max error", err.max(), "rad")
    assert err.max() <= 1e-9 and got.min() >= 0 and got.max() <= 2 * np.pi


def test_angle_on_the_boundaries():
    capi = _capi()
    t8 = float(ref.T8)
    qs = [np.nextafter(t8, 0.0), t8, np.nextafter(t8, 1.0)]
    tiny = [5e-324, 1e-310, 2.2250738585072014e-308]  # denormal m (and the smallest normal)
    mags = [1e-3, 1.0, 7.0, 1e3]
    s, t = [], []
    for m in mags:
        for sx in (1.0, -1.0):
            for sy in (1.0, -1.0):
                s += [sx * m, sx * m, 0.0, -0.0, sx * m, sx * m]       # S = +-T, S = +-0, T = +-0
                t += [sy * m, -sy * m, sy * m, sy * m, 0.0, -0.0]
                for q in qs:                                           # q on either side of tan(pi/8), in both octants
                    s += [sx * m, sx * m * q]
                    t += [sy * m * q, sy * m]
                for d in tiny:                                         # denormal m
                    s += [sx * m, sx * d]
                    t += [sy * d, sy * m]
    s, t = np.array(s), np.array(t)
    got = capi.cyl_angle_host(s, t)
    assert got.tobytes() == ref.angle(s, t).tobytes()
    assert _wrap_error(got, s, t).max() <= 1e-9 and got.min() >= 0 and got.max() <= 2 * np.pi
    # -0 is not < 0: no unfolding; a quotient that underflows under T < 0 gives 2 pi itself
    assert capi.cyl_angle_host([1.0, -1.0], [-0.0, -0.0]).tolist() == [0.0, np.pi]
    assert capi.cyl_angle_host([1.0], [-5e-324])[0] == 2 * np.pi
    assert np.isnan(capi.cyl_angle_host([0.0], [0.0])[0])


def _case_frames(item):
    """the fitted frame and a coarser, narrower one that cuts rows by its raster and its window"""
    fr = dict(item["frame"])
    small = dict(fr, gsd=float(np.float32(0.05)), width=max(2, int(fr["width"] * 0.2 * 0.7)), height=max(2, int(fr["height"] * 0.2 * 0.8)),
                 d_min=float(np.float32(-0.001)), d_max=float(np.float32(0.05)))
    return fr, small


@pytest.mark.parametrize("fam", [0, 3])
def test_host_twin_equals_the_restatement(fitted, fam):
    capi = _capi()
    item = fitted[(fam, 1)]
    xyz = item["scene"]["xyz"]
    n = len(xyz)
    rgb = ref.hash_colours(n)
    label = (np.arange(n) % 251).astype(np.uint8)
    has = (np.arange(n) % 7 != 0).astype(np.uint8)
    for fr in _case_frames(item):
        cut_raster, cut_window = ref.cuts(fr, xyz)
        for fill in (0, 2):
            want = ref.ortho(fr, xyz, rgb, label, has, index_base=5, fill_radius=fill)
            got = capi.ortho_cyl_host(fr, xyz, rgb, label, has, index_base=5, fill_radius=fill)
            print(fr["width"], fr["height"], "fill", fill, "contributors", want["contributors"], "occupied", want["occupied"], "filled",
                  want["filled"], "cut", cut_raster, cut_window, "shared pixels", int((want["per_pixel"] >= 2).sum()))
            assert want["contributors"] > 1000 and (want["per_pixel"] >= 2).any() and (fill == 0 or want["filled"] > 0)
            assert ref.same(got, want, with_label=True) is None
            assert (got["contributors"], got["occupied"], got["filled"]) == (want["contributors"], want["occupied"], want["filled"])
    fr, small = _case_frames(item)
    assert ref.cuts(fr, xyz) == (0, 0) and min(ref.cuts(small, xyz)) > 0  # (the second frame cuts both ways)


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_fit_equals_the_restatement_and_meets_the_ground_truth(fitted):
    capi = _capi()
    for (fam, seed), item in fitted.items():
        sc, want, ws = item["scene"], item["frame"], item["stats"]
        # the restatement alone against the ground truth
        axis_err = float(np.arccos(min(1.0, abs(ws["axis"] @ sc["axis"]))))
        dc = ws["c0"] - sc["centre"]
        dc = dc - (dc @ sc["axis"]) * sc["axis"]
        print(fam, seed, "axis %.2e rad  centre %.2e m  R %.2e m  rms/sigma %.4f" % (axis_err, np.linalg.norm(dc), abs(ws["R"] - sc["R"]),
                                                                                    ws["rms"] / SIGMA))
        assert axis_err <= 2e-3 and np.linalg.norm(dc) <= 5e-4 and abs(ws["R"] - sc["R"]) <= 5e-4 and 0.9 <= ws["rms"] / SIGMA <= 1.1
        # the library against the restatement
        gf, gs = capi.cyl_fit_host(sc["xyz"], item["normal"], GSD)
        g = gf.as_dict()
        assert gs["rows"] == ws["rows"] == len(sc["xyz"])
        for k in ("rms", "dev_min", "dev_max", "arc", "ev0", "ev1", "ev2"):
            assert _rel(gs[k], ws[k]) <= 1e-9, (fam, seed, k, gs[k], ws[k])
        for k in ("a", "e", "b"):
            assert np.abs(np.array(g[k]) - np.array(want[k])).max() <= 1e-6, (fam, seed, k)
        # (c, R and the window are float32 in the frame: equal, or one rounding apart where an fp64 value sits on a tie)
        assert np.abs(np.array(g["c"]) - np.array(want["c"])).max() <= 1e-6 and _rel(g["radius"], want["radius"]) <= 1.2e-7
        assert (g["width"], g["height"], g["side"]) == (want["width"], want["height"], want["side"])
        assert abs(g["d_min"] - want["d_min"]) <= 1e-6 and abs(g["d_max"] - want["d_max"]) <= 1e-6


def test_every_fitted_row_contributes_and_the_seam_lies_in_the_gap(fitted):
    capi = _capi()
    for (fam, seed), item in fitted.items():
        sc = item["scene"]
        N, R, H, arc, _ = FAMILIES[fam]
        gf, gs = capi.cyl_fit_host(sc["xyz"], item["normal"], GSD)
        g = gf.as_dict()
        ok, _, _ = ref.project(g, sc["xyz"])
        assert ok.all(), (fam, seed, int((~ok).sum()))
        around = 2 * np.pi * g["radius"]
        if arc >= 2 * np.pi:  # the closed ring
            assert g["width"] == int(np.ceil(around / g["gsd"])) and gs["arc"] > 2 * np.pi - 0.05
        else:  # the seam lies in the gap: no row within a pixel of it on either side, and the raster ends before it comes round
            _, x, _, _ = ref.coords(g, sc["xyz"])
            assert x.min() >= 1.0 and x.max() < g["width"] - 1 and g["width"] * g["gsd"] < around - 0.5 * (2 * np.pi - arc) * R
            assert abs(gs["arc"] - arc) < 0.02


def test_handedness_for_a_viewer_inside_and_outside(fitted):
    capi = _capi()
    item = fitted[(0, 1)]
    sc = item["scene"]
    inside = sc["centre"] + 0.3 * sc["rot"][:, 0] + 0.5 * sc["axis"]
    outside = sc["centre"] + 4.0 * sc["rot"][:, 0] - 0.5 * sc["axis"]
    for viewer, side in ((inside, 1), (outside, -1), (None, -1)):
        gf, _ = capi.cyl_fit_host(sc["xyz"], item["normal"], GSD, viewer=viewer)
        g = gf.as_dict()
        want, _ = ref.fit(sc["xyz"], item["normal"], GSD, viewer=viewer)
        a, e, b = (np.array(g[k], np.float64) for k in ("a", "e", "b"))
        assert g["side"] == side == want["side"]
        assert np.abs(np.cross(e, b) - side * a).max() <= 1e-6
        assert a[np.argmax(np.abs(a))] < 0
        assert np.abs(b - np.array(want["b"])).max() <= 1e-6
        # seen from `side`, image x (towards b at theta = 0) x image y (a) is the viewing direction: -e from outside, +e from inside
        assert np.abs(np.cross(b, a) - side * e).max() <= 1e-6
        assert ref.project(g, sc["xyz"])[0].all()


def test_an_asymmetric_mark_reads_unmirrored_from_either_side(fitted):
    """an L on the surface: a stem that runs UP the structure from a corner and a foot that runs to the viewer's RIGHT of it.
    In the picture the stem's end lies above the corner (a smaller row) and the foot's end right of it (a larger column)."""
    capi = _capi()
    item = fitted[(0, 1)]  # the half cylinder of R 1 over scene angles [0, pi)
    sc = item["scene"]
    rot, centre = sc["rot"], sc["centre"]
    a0 = capi.cyl_fit_host(sc["xyz"], item["normal"], GSD)[0].as_dict()["a"]
    up = -np.array(a0) if abs(np.array(a0) @ rot[:, 2]) > 0.99 else None  # rows run along +a, downwards: "up" is -a
    assert up is not None
    phi = np.pi / 2  # the mark's corner, in the middle of the arc
    r_hat = np.cos(phi) * rot[:, 0] + np.sin(phi) * rot[:, 1]
    corner = centre + 1.0 * r_hat
    for viewer, side in ((centre + 0.2 * r_hat, 1), (centre + 4.0 * r_hat, -1)):
        look = side * r_hat  # from inside the viewer looks outwards at the corner, from outside inwards
        right = np.cross(look, up)  # the viewer's right: look x up for x right, y down, z forward (up = -y)
        right /= np.linalg.norm(right)
        rel = np.stack([corner, corner + 0.3 * up, corner + 0.2 * right]) - centre
        axial = (rel @ up)[:, None] * up
        radial = rel - axial
        marks = centre + axial + radial / np.linalg.norm(radial, axis=1, keepdims=True)  # (the foot's end back onto R = 1)
        gf, _ = capi.cyl_fit_host(sc["xyz"], item["normal"], GSD, viewer=viewer)
        g = gf.as_dict()
        assert g["side"] == side
        ok, pixel, _ = ref.project(g, marks.astype(np.float32))
        assert ok.all()
        row, col = pixel // g["width"], pixel % g["width"]
        print("side", side, "corner", (row[0], col[0]), "stem end", (row[1], col[1]), "foot end", (row[2], col[2]))
        assert row[1] < row[0] - 20 and abs(col[1] - col[0]) <= 1, "the stem runs up the picture"
        assert col[2] > col[0] + 10 and abs(row[2] - row[0]) <= 1, "the foot runs to the right"


def _sphere(n, radius, seed, cap=None):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    if cap is not None:
        d[:, 2] = np.abs(d[:, 2]) + cap * np.linalg.norm(d[:, :2], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (ref.CENTRE + radius * d).astype(np.float32), d.astype(np.float32)


def test_a_sphere_and_a_cap_are_not_cylindrical():
    """the fit goes through on both (their normals have every direction) and the rms says what they are: 0.112 m and 0.050 m"""
    capi = _capi()
    max_rms = 0.01  # (FA7's threshold as the pipeline and the command line default it)
    for cap, low, high in ((None, 0.10, 0.125), (1.0, 0.04, 0.06)):
        xyz, normal = _sphere(8000, 0.5, 21, cap)
        _, gs = capi.cyl_fit_host(xyz, normal, GSD)
        _, ws = ref.fit(xyz, normal, GSD)
        print("sphere" if cap is None else "cap", "rms", gs["rms"], ws["rms"])
        assert gs["rms"] > max_rms and low < ws["rms"] < high and _rel(gs["rms"], ws["rms"]) <= 1e-9


def _good():
    return ref.frame((0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, 0), 1.0, 0.01, 100, 100, -0.5, 0.5, -1)


def test_frame_refusals():
    capi = _capi()
    xyz = np.array([[1.0, 0.1, 0.5]], np.float32)
    rgb = np.zeros((1, 3), np.uint8)
    assert capi.ortho_cyl_host(_good(), xyz, rgb)["contributors"] == 1
    nan = float("nan")
    bad = (("c", (nan, 0, 0), "finite"), ("radius", float("inf"), "finite"), ("gsd", 5e-5, "gsd"), ("gsd", 1.5, "gsd"),
           ("radius", 0.04, "radius"), ("radius", 1001.0, "radius"), ("side", 0, "side"), ("side", 2, "side"),
           ("d_max", -0.5, "window"), ("width", 0, "width"), ("height", -3, "width"),
           ("e", (0.999, 0.05, 0), "orthonormal"), ("a", (0, 0, 1), "e x b = side a"), ("b", (0, -1, 0), "e x b = side a"),
           ("side", 1, "e x b = side a"), ("width", 630, "circumference"))
    for key, value, word in bad:
        with pytest.raises(capi.PcpError) as e:
            capi.ortho_cyl_host(dict(_good(), **{key: value}), xyz, rgb)
        assert e.value.code == capi.PCP_ERR_INVALID and word in str(e.value) and "pcp_ortho_cyl_host" in str(e.value), (key, value, str(e.value))
    assert capi.ortho_cyl_host(dict(_good(), width=629), xyz, rgb)["contributors"] == 1
    big = dict(_good(), radius=100.0, width=20000)
    with pytest.raises(capi.PcpError) as e:
        capi.ortho_cyl_host(big, xyz, rgb)
    assert e.value.code == capi.PCP_ERR_RANGE and "fits at gsd 0.0122" in str(e.value)
    for kw, code in ((dict(fill_radius=-1), capi.PCP_ERR_INVALID), (dict(fill_radius=1025), capi.PCP_ERR_INVALID),
                     (dict(index_base=-1), capi.PCP_ERR_RANGE), (dict(index_base=2 ** 32 - 1), capi.PCP_ERR_RANGE)):
        with pytest.raises(capi.PcpError) as e:
            capi.ortho_cyl_host(_good(), xyz, rgb, **kw)
        assert e.value.code == code and "pcp_ortho_cyl_host" in str(e.value)
    L = capi.load()
    assert L.pcp_ortho_cyl_host(None, C.c_int64(0), *([None] * 4), C.c_int64(0), C.c_int32(0), *([None] * 9)) == capi.PCP_ERR_INVALID
    assert L.pcp_cyl_angle_host(C.c_int64(2), None, None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_cyl_angle_host(C.c_int64(-1), None, None, None) == capi.PCP_ERR_INVALID


def test_fit_refusals(fitted):
    capi = _capi()
    item = fitted[(3, 1)]
    xyz, normal = item["scene"]["xyz"], item["normal"]
    for gsd in (5e-5, 2.0, float("nan")):
        with pytest.raises(capi.PcpError) as e:
            capi.cyl_fit_host(xyz, normal, gsd)
        assert e.value.code == capi.PCP_ERR_INVALID and "gsd" in str(e.value)
    with pytest.raises(capi.PcpError) as e:
        capi.cyl_fit_host(xyz, normal, GSD, viewer=(0, float("inf"), 0))
    assert e.value.code == capi.PCP_ERR_INVALID and "viewer" in str(e.value)
    # fewer than 16 rows: by n, by has, by invalid normals
    has = np.zeros(len(xyz), np.uint8)
    has[:15] = 1
    zeroed = normal.copy()
    zeroed[15:] = 0
    for kw in (dict(xyz=xyz[:15], normal=normal[:15]), dict(xyz=xyz, normal=normal, has=has), dict(xyz=xyz, normal=zeroed)):
        with pytest.raises(capi.PcpError) as e:
            capi.cyl_fit_host(gsd=GSD, **kw)
        assert e.value.code == capi.PCP_ERR_RANGE and "15 rows" in str(e.value) and "16" in str(e.value)
    has[:16] = 1
    assert capi.cyl_fit_host(xyz, normal, GSD, has=has)[1]["rows"] == 16
    # all normals parallel: a plane has no axis
    rng = np.random.default_rng(3)
    flat = np.stack([rng.random(500), rng.random(500), np.zeros(500)], axis=1).astype(np.float32)
    up = np.tile(np.array([0, 0, 1], np.float32), (500, 1))
    with pytest.raises(capi.PcpError) as e:
        capi.cyl_fit_host(flat, up, GSD)
    assert e.value.code == capi.PCP_ERR_RANGE and "no direction" in str(e.value)
    # the radius: the same ring scaled down to R = 0.02 and up to R = 2000
    centre = item["scene"]["centre"]
    for scale, gsd in ((0.05, 0.001), (5000.0, 1.0)):
        with pytest.raises(capi.PcpError) as e:
            capi.cyl_fit_host(((xyz - centre) * scale).astype(np.float32), normal, gsd)
        assert e.value.code == capi.PCP_ERR_RANGE and "radius" in str(e.value), str(e.value)
    # the raster: R = 40 at 1 mm is 251 k pixels round
    with pytest.raises(capi.PcpError) as e:
        capi.cyl_fit_host(((xyz - centre) * 100.0).astype(np.float32), normal, 0.001)
    assert e.value.code == capi.PCP_ERR_RANGE and "fits at gsd" in str(e.value)
    fit_gsd = float(str(e.value).split("fits at gsd")[1].split()[0])
    assert capi.cyl_fit_host(((xyz - centre) * 100.0).astype(np.float32), normal, fit_gsd * 1.001)[0].width <= 16384
    L = capi.load()
    assert L.pcp_cyl_fit_host(C.c_int64(4), None, None, None, None, C.c_float(0.01), None, None) == capi.PCP_ERR_INVALID


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    assert callable(capi.Context.ortho_begin_cyl) and callable(capi.ortho_cyl_host) and callable(capi.cyl_fit_host)
    assert callable(capi.cyl_angle_host) and callable(capi.cyl_frame)
    assert lib.pcp_abi_version() == 6 and capi.K_COUNT == 13
    assert C.sizeof(capi.CylFrame) == 76 and C.sizeof(capi.OrthoFrame) == 68 and len(capi.CY_STATS) == 8


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  ' + "\n  ".join(f"(void){s};" for s in NEW) +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && sizeof(pcp_cyl_frame) == 76 && sizeof(pcp_ortho_frame) == 68 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["ortho_cyl_selftest"]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "ortho_cyl_selftest.cpp")
    exe = str(tmp_path / "ortho_cyl_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr
