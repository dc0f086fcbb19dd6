"""Orthophotos of unrolled maps without a GPU ("Orthophotos of unrolled maps", CT1, CT2, CT5, CT7): pcp_cyl_sincos_host
and pcp_ortho_texture_points_cyl_host against the restatement in _ortho_cyl_texture_ref.py by exact equality of the bytes, the
sine and cosine within 1e-12 of numpy's, the surface points through CY2 and back, the refusals, the symbols, the header as C and
the stand-alone self-test plain and under the host sanitizers."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _ortho_cyl_ref as cyl
import _ortho_cyl_texture_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_ortho_texture_cyl", "pcp_ortho_texture_points_cyl_host", "pcp_cyl_sincos_host")
MAX_STEP = 0.002  # metres: about the noise of neighbouring pixels' depths on either scene, so it cuts some neighbours and keeps some


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


def _neighbours(t):
    t = np.asarray(t, np.float64)
    return np.concatenate([t, np.nextafter(t, 64.0), np.nextafter(t, 0.0)])


def _crossings():
    """the angles below 64 where theta kTwoOverPi + 0.5 crosses an integer: for every k the last angle that gives k and the
    first that gives k + 1"""
    out = []
    for k in range(40):
        t = np.float64((k + 0.5) / ref.TWO_OVER_PI)
        while ref.reduce(t)[0] > k:
            t = np.nextafter(t, 0.0)
        while ref.reduce(np.nextafter(t, 64.0))[0] == k:
            t = np.nextafter(t, 64.0)
        assert ref.reduce(t)[0] == k and ref.reduce(np.nextafter(t, 64.0))[0] == k + 1
        out += [t, np.nextafter(t, 64.0)]
    return np.array(out)


def _angles():
    rng = np.random.default_rng(20)
    special = np.concatenate([_neighbours([j * cyl.PI4 for j in range(9)]), _neighbours(_crossings()), [0.0, 5e-324]])
    special = special[(special >= 0) & (special < 64)]
    return dict(ring=rng.uniform(0, 2 * np.pi, 1_000_000), past=rng.uniform(2 * np.pi, 2 * np.pi + 20, 10_000), special=special)


def _identity_error(s, c):
    """|s^2 + c^2 - 1| of the returned doubles, not of a float64 evaluation of it (whose three roundings alone reach 3e-16): in
    the extended format where numpy has one with a 64-bit significand, else exactly, in rationals, on a sample"""
    if np.finfo(np.longdouble).eps <= 2.0 ** -63:
        ls, lc = s.astype(np.longdouble), c.astype(np.longdouble)
        return float(np.abs(ls * ls + lc * lc - 1).max())
    pick = np.linspace(0, len(s) - 1, min(len(s), 20000)).astype(np.int64)
    return max(abs(float(Fraction(float(s[i])) ** 2 + Fraction(float(c[i])) ** 2 - 1)) for i in pick)


@pytest.mark.parametrize("which", ["ring", "past", "special"])
def test_sincos_equals_the_restatement_and_numpy(which):
    capi = _capi()
    theta = _angles()[which]
    s, c = capi.cyl_sincos_host(theta)
    rs, rc = ref.sincos(theta)
    assert s.tobytes() == rs.tobytes() and c.tobytes() == rc.tobytes()
    err = max(np.abs(s - np.sin(theta)).max(), np.abs(c - np.cos(theta)).max())
    ident = _identity_error(s, c)
    k, r = ref.reduce(theta)
    print(f"{which}: {len(theta)} angles, k up to {k.max()}, |r| up to pi/4 + {np.abs(r).max() - cyl.PI4:.3g}, worst error {err:.3g}, "
          f"worst |s^2 + c^2 - 1| {ident:.3g}")
    # (CT1: the quadrant is chosen from u = theta kTwoOverPi + 0.5 after three roundings of 2^-53 relative each, u < 41.3, and
    # a change of u by du moves r by (pi / 2) du: |r| <= pi/4 + (pi / 2) 41.3 3 2^-53 < pi/4 + 2^-45)
    assert np.abs(r).max() <= cyl.PI4 + 2.0 ** -45
    assert err <= 1e-12
    assert ident <= 4e-16


def test_sincos_exact_values_and_refusals():
    capi = _capi()
    s, c = capi.cyl_sincos_host([0.0, 5e-324, cyl.PI2, cyl.PI, 3 * cyl.PI2, cyl.TWO_PI])
    assert s.tolist() == [0.0, 5e-324, 1.0, 0.0, -1.0, 0.0] and c.tolist() == [1.0, 1.0, 0.0, -1.0, 0.0, 1.0]
    assert len(capi.cyl_sincos_host([])[0]) == 0
    for bad in (-1e-300, -0.5, 64.0, 1e300, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(capi.PcpError) as e:
            capi.cyl_sincos_host([1.0, bad])
        assert e.value.code == capi.PCP_ERR_INVALID and "pcp_cyl_sincos_host" in str(e.value) and "theta[1]" in str(e.value), str(e.value)
    assert len(capi.cyl_sincos_host([np.nextafter(64.0, 0.0)])[0]) == 1
    L = capi.load()
    one = np.ones(1)
    assert L.pcp_cyl_sincos_host(C.c_int64(-1), capi._ptr(one), capi._ptr(one), capi._ptr(one)) == capi.PCP_ERR_INVALID
    assert "negative n" in L.pcp_last_error(None).decode()
    for args in ((None, capi._ptr(one), capi._ptr(one)), (capi._ptr(one), None, capi._ptr(one)), (capi._ptr(one), capi._ptr(one), None)):
        assert L.pcp_cyl_sincos_host(C.c_int64(1), *args) == capi.PCP_ERR_INVALID
    assert L.pcp_cyl_sincos_host(C.c_int64(0), None, None, None) == capi.PCP_OK


@pytest.fixture(scope="module")
def maps():
    """the two scenes' maps by the host twin of the device's (pcp_ortho_cyl_host, every row a contributor; the vault filled at
    R = 2, the pier not filled, so that both keep holes): computed once, left unchanged"""
    capi = _capi()
    pts = ref.scene_points()
    rgb = np.zeros((len(pts), 3), np.uint8)
    out = {}
    for name, fr in ref.scene_frames().items():
        m = capi.ortho_cyl_host(fr, pts, rgb, fill_radius=ref.SCENE_FILL[name])
        for v in m.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        assert m["occupied"] >= 10000 and (m["filled"] >= 100) == (ref.SCENE_FILL[name] > 0) and (m["status"] == 0).sum() >= 100
        out[name] = (fr, m)
    assert out["vault"][0]["side"] == 1 and out["pier"][0]["side"] == -1
    assert out["pier"][0]["width"] == int(np.ceil(2 * np.pi * out["pier"][0]["radius"] / out["pier"][0]["gsd"])), "a closed ring"
    assert out["vault"][0]["width"] * out["vault"][0]["gsd"] < 0.4 * 2 * np.pi * out["vault"][0]["radius"], "an open arc"
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 4, 16])
@pytest.mark.parametrize("name", ["vault", "pier"])
def test_host_points_equal_the_restatement(maps, name, k):
    capi = _capi()
    fr, m = maps[name]
    W, H = fr["width"], fr["height"]
    rect = (W - 60, 9, 60, 31) if k == 16 else None  # (the raster's last columns, where theta is largest: 2 pi on the ring)
    w, h = (W, H) if rect is None else rect[2:]
    results = {}
    for interpolate in (False, True):
        for max_step in (MAX_STEP, 100.0):
            ok, xyz = ref.surface(fr, m["source"], m["depth"], k, interpolate, max_step, rect)
            got = capi.ortho_texture_points_cyl_host(fr, m["source"], m["depth"], k, interpolate, max_step, rect)
            assert got["ok"].shape == (h * k, w * k) and got["xyz"].shape == got["ok"].shape + (3,)
            assert got["ok"].tobytes() == ok.astype(np.uint8).tobytes()
            assert got["xyz"].tobytes() == xyz.tobytes(), (k, interpolate, max_step)
            results[interpolate, max_step] = xyz
    n = int(ok.sum())
    off, cut, free = results[False, MAX_STEP], results[True, MAX_STEP], results[True, 100.0]
    assert results[False, 100.0].tobytes() == off.tobytes()
    moved_cut, moved_free = int((cut != off).any(axis=2).sum()), int((free != off).any(axis=2).sum())
    print(f"{name} k {k}: {n} surface pixels of {ok.size}, moved by the interpolation: {moved_cut} at {MAX_STEP}, {moved_free} at 100")
    assert n >= 1000 and n < ok.size, "surface and holes"
    if k == 1:
        assert moved_cut == 0 and moved_free == 0, "a fine pixel at its parent's centre has the parent's depth"
    else:
        assert 0 < moved_cut < moved_free, "max_step cuts some neighbours and not all"
    # the whole against rectangles: 2 x 2 of them, cut where no side is a multiple of anything
    if rect is None and k in (2, 3):
        cx, cy = 131, 29
        whole = capi.ortho_texture_points_cyl_host(fr, m["source"], m["depth"], k, True, MAX_STEP)
        parts = [capi.ortho_texture_points_cyl_host(fr, m["source"], m["depth"], k, True, MAX_STEP, r)
                 for r in ((0, 0, cx, cy), (cx, 0, W - cx, cy), (0, cy, cx, H - cy), (cx, cy, W - cx, H - cy))]
        for key in ("xyz", "ok"):
            joined = np.concatenate([np.concatenate([parts[0][key], parts[1][key]], axis=1),
                                     np.concatenate([parts[2][key], parts[3][key]], axis=1)], axis=0)
            assert joined.tobytes() == whole[key].tobytes(), key


@pytest.mark.parametrize("name", ["vault", "pier"])
def test_surface_points_go_through_cy2_and_come_back(maps, name):
    """Every surface point, taken through the restatement of CY2 (_ortho_cyl_ref.coords: no exported call returns the pixel and
    depth of a single point), lands in its parent map pixel, at a depth within 1e-5 m of the one it was made from: the fp32
    rounding of p is below 1e-6 m per coordinate at coordinates below 16 m, a few such roundings add up, and the margin to a
    pixel's edge is gsd / 2k >= 6e-4 m (gsd >= 5 mm, k <= 4).  The stated exception (CT2): a closed ring's last column is wider
    than what is left of the circumference (CY1 allows width gsd <= 2 pi R + gsd), and a fine pixel of it whose centre lies past
    2 pi R is the point at theta - 2 pi, which CY2 puts into the first columns: those are checked to do just that."""
    capi = _capi()
    fr, m = maps[name]
    assert fr["gsd"] >= 0.005
    for k in (1, 2, 3, 4):
        got = capi.ortho_texture_points_cyl_host(fr, m["source"], m["depth"], k, True, MAX_STEP)
        ok = got["ok"].astype(bool)
        _, d = ref.fine_depth(fr, m["source"], m["depth"], k, True, MAX_STEP)
        assert np.abs(got["xyz"][ok]).max() < 16.0
        rows, cols = np.nonzero(ok)
        usable, x, y, depth = cyl.coords(fr, got["xyz"][ok])
        assert usable.all()
        worst = float(np.abs(depth.astype(np.float64) - d[ok].astype(np.float64)).max())
        around = 2 * np.pi * fr["radius"]
        past = (cols + 0.5) / k * fr["gsd"] > around
        print(f"{name} k {k}: {len(rows)} points, {int(past.sum())} past the seam, worst depth error {worst:.3g} m")
        assert past.any() == (name == "pier") and (cols[past] // k == fr["width"] - 1).all()
        col = np.floor(x).astype(np.int64)
        assert (col[~past] == cols[~past] // k).all() and (np.floor(y).astype(np.int64) == rows // k).all()
        assert (col[past] == np.floor(((cols[past] + 0.5) / k * fr["gsd"] - around) / fr["gsd"])).all() and (col[past] == 0).all()
        assert worst <= 1e-5


def test_no_surface_where_rho_is_not_above_zero():
    """a map whose depths reach the axis and beyond (a depth window wider than the radius allows them): rho = R + side d <= 0 is
    no surface, for both sides"""
    capi = _capi()
    for side in (1, -1):
        a, e = np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0])
        fr = cyl.frame([1.0, 2.0, 3.0], a, e, side * np.cross(a, e), 0.25, 0.01, 40, 8, -1.0, 1.0, side)
        source = np.arange(320, dtype=np.int32).reshape(8, 40)
        depth = np.zeros((8, 40), np.float32)
        depth[:, 10:20] = -side * 0.25   # rho == 0
        depth[:, 20:30] = -side * 0.5    # rho < 0
        depth[:, 30:] = -side * 0.2499   # just off the axis
        for k in (1, 3):
            got = capi.ortho_texture_points_cyl_host(fr, source, depth, k, False, 0.05)
            ok, xyz = ref.surface(fr, source, depth, k, False, 0.05)
            assert got["ok"].tobytes() == ok.astype(np.uint8).tobytes() and got["xyz"].tobytes() == xyz.tobytes()
            cols = np.arange(40 * k) // k
            assert (got["ok"][:, (cols >= 10) & (cols < 30)] == 0).all() and not got["xyz"][:, (cols >= 10) & (cols < 30)].any()
            assert (got["ok"][:, (cols < 10) | (cols >= 30)] == 1).all()


def test_refusals_by_code_and_message(maps):
    capi = _capi()
    fr, m = maps["pier"]
    W, H = fr["width"], fr["height"]
    L = capi.load()

    def call(scale=2, interpolate=True, max_step=0.05, rect=None, frame=fr, views=1):
        f = capi.cyl_frame(frame)
        p = capi.ortho_texture_params(scale, views, interpolate, max_step, rect)
        same = frame["width"] == W and frame["height"] == H
        src = np.ascontiguousarray(m["source"] if same else np.zeros((frame["height"], frame["width"]), np.int32))
        dep = np.ascontiguousarray(m["depth"] if same else np.zeros((frame["height"], frame["width"]), np.float32))
        one = np.zeros(16, np.float32)  # (a refused call writes nothing)
        rc = L.pcp_ortho_texture_points_cyl_host(C.byref(f), C.byref(p), capi._ptr(src), capi._ptr(dep), capi._ptr(one), None)
        assert not one.any()
        return rc, L.pcp_last_error(None).decode()

    for kw in (dict(scale=0), dict(scale=17), dict(views=0), dict(views=6), dict(rect=(0, 0, 10, 0)), dict(rect=(W - 9, 0, 10, 10)),
               dict(rect=(0, H - 9, 10, 10)), dict(rect=(-1, 0, 10, 10)), dict(rect=(3, 0, 0, 0)), dict(max_step=0.0),
               dict(max_step=float("nan"))):
        rc, msg = call(**kw)
        assert rc == capi.PCP_ERR_INVALID and "pcp_ortho_texture_points_cyl_host" in msg, (kw, rc, msg)
    # CY1's frame rules come first, by their own words
    for change, needle in ((dict(side=0), "side"), (dict(radius=0.01), "radius"), (dict(gsd=2.0), "gsd"), (dict(width=W + 2), "circumference"),
                           (dict(b=fr["e"]), "orthonormal")):
        rc, msg = call(frame=dict(fr, **change), scale=0)
        assert rc == capi.PCP_ERR_INVALID and needle in msg and "pcp_ortho_texture_points_cyl_host" in msg, (change, msg)
    big = dict(fr, radius=900.0, gsd=0.01, width=16384, height=4096)
    rc, msg = call(scale=3, frame=big)
    assert rc == capi.PCP_ERR_RANGE and "largest scale that fits the rectangle is 2" in msg, msg
    rc, msg = call(frame=dict(big, width=16385))
    assert rc == capi.PCP_ERR_RANGE
    # NULL arguments, a source image that names a pixel outside the map, layers of another shape, nullable outputs
    f, p = capi.cyl_frame(fr), capi.ortho_texture_params(2)
    src, dep = np.ascontiguousarray(m["source"]), np.ascontiguousarray(m["depth"])
    assert L.pcp_ortho_texture_points_cyl_host(None, C.byref(p), capi._ptr(src), capi._ptr(dep), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_ortho_texture_points_cyl_host(C.byref(f), None, capi._ptr(src), capi._ptr(dep), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_ortho_texture_points_cyl_host(C.byref(f), C.byref(p), None, capi._ptr(dep), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_ortho_texture_points_cyl_host(C.byref(f), C.byref(p), capi._ptr(src), None, None, None) == capi.PCP_ERR_INVALID
    bad = m["source"].copy()
    bad[5, 5] = W * H
    with pytest.raises(capi.PcpError) as e:
        capi.ortho_texture_points_cyl_host(fr, bad, m["depth"], 2)
    assert e.value.code == capi.PCP_ERR_INVALID and "names no pixel" in str(e.value)
    with pytest.raises(ValueError):
        capi.ortho_texture_points_cyl_host(fr, m["source"][:-1], m["depth"][:-1], 2)
    assert L.pcp_ortho_texture_points_cyl_host(C.byref(f), C.byref(p), capi._ptr(src), capi._ptr(dep), None, None) == capi.PCP_OK


def test_pipeline_refuses_texture_cylinders_without_its_companions():
    from pointcloudprocessor_amd import pipeline

    col = pipeline.PointCloudColorizer(None)
    for kw in (dict(texture_cylinders=True), dict(texture_cylinders=True, cylinders=True), dict(texture_cylinders=True, texture=dict(scale=2))):
        with pytest.raises(ValueError) as e:
            col.ortho_maps_by_facet(0.01, **kw)
        assert "texture_cylinders" in str(e.value) and "texture" in str(e.value) and "cylinders=True" in str(e.value)


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    assert callable(capi.Context.ortho_texture_cyl) and callable(capi.ortho_texture_points_cyl_host) and callable(capi.cyl_sincos_host)
    assert lib.pcp_abi_version() == 6 and capi.K_COUNT == 13
    assert C.sizeof(capi.CylFrame) == 76 and C.sizeof(capi.OrthoTextureParams) == 32


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  ' + "\n  ".join(f"(void){s};" for s in NEW) +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && sizeof(pcp_cyl_frame) == 76 && sizeof(pcp_ortho_texture_params) == 32 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_plain_and_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own: the project's build of it, and one with the address and
    undefined-behaviour sanitizers, on the CPU."""
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["ortho_cyl_texture_selftest"]
    plain = subprocess.run([exe], capture_output=True, text=True)
    assert plain.returncode == 0 and "0 mismatches" in plain.stdout, plain.stdout + plain.stderr
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "ortho_cyl_texture_selftest.cpp")
    san_exe = str(tmp_path / "ortho_cyl_texture_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", san_exe], check=True, capture_output=True)
    san = subprocess.run([san_exe], capture_output=True, text=True)
    assert san.returncode == 0 and "0 mismatches" in san.stdout, san.stdout + san.stderr
