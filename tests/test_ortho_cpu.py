"""The orthographic maps without a GPU ("Orthographic maps"): pcp_ortho_host against the restatement in
_ortho_ref.py on the scenes test_ortho_gpu.py uses, ord()'s order, the refusals, the symbols, the stand-alone selftest plain and
under the host sanitizers, and pcp_ortho_fit_frame_host on an exact tilted plane.  Every comparison is exact equality unless
said otherwise."""
import os
import re
import subprocess

import numpy as np
import pytest

import _ortho_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pcp_ortho_begin", "pcp_ortho_add", "pcp_ortho_add_packed", "pcp_ortho_finish", "pcp_ortho_fetch", "pcp_ortho_stats",
       "pcp_ortho_end", "pcp_ortho_host", "pcp_ortho_fit_frame_host"]

_SCENE = {}


def _scene():
    if not _SCENE:
        b = ref.base_scene()
        for v in b.values():
            v.setflags(write=False)
        _SCENE.update(b)
    return _SCENE


def _check(capi, fr, xyz, rgb, fill_radius=0, **kw):
    want = ref.ortho(fr, xyz, rgb, fill_radius=fill_radius, **kw)
    got = capi.ortho_host(fr, xyz, rgb, fill_radius=fill_radius, **kw)
    bad = ref.same(got, want, with_label=kw.get("label") is not None)
    assert bad is None, f"{bad} differs"
    assert (got["contributors"], got["occupied"], got["filled"]) == (want["contributors"], want["occupied"], want["filled"])
    return want


@pytest.mark.parametrize("gsd,radius", [(0.05, 0), (0.05, 2), (0.02, 4), (0.2, 0), (0.2, 4)])
def test_host_equals_the_restatement(gsd, radius):
    from pointcloudprocessor_amd import capi

    s = _scene()
    want = _check(capi, ref.down_frame(gsd), s["xyz"], s["rgb"], fill_radius=radius)
    pp = want["per_pixel"]
    print(f"gsd {gsd} R {radius}: occupied {want['occupied']} multi {(pp >= 2).sum()} max {pp.max()} ties {want['ties']} "
          f"filled {want['filled']} empty {(want['status'] == 0).sum()}")
    if (gsd, radius) == (0.05, 2):
        assert (pp >= 2).sum() >= 1000 and want["ties"] >= 50 and want["filled"] >= 1000 and (want["status"] == 0).sum() >= 1000


def test_host_depths_of_both_signs_window_labels_and_has():
    from pointcloudprocessor_amd import capi

    s = _scene()
    inside = ref.down_frame(0.05, d_min=-100.0, d_max=100.0, oz=1.5)
    want = _check(capi, inside, s["xyz"], s["rgb"], fill_radius=1)
    direct = want["status"] == 1
    assert (want["depth"][direct] < 0).sum() >= 100 and (want["depth"][direct] > 0).sum() >= 100, "both signs win pixels"
    cut = _check(capi, ref.down_frame(0.05, d_min=6.0), s["xyz"], s["rgb"])
    assert 0 < cut["contributors"] < len(s["xyz"]), "the window leaves the floor out"
    rng = np.random.default_rng(3)
    label = rng.integers(0, 256, len(s["xyz"])).astype(np.uint8)
    has = (rng.random(len(s["xyz"])) < 0.7).astype(np.uint8)
    _check(capi, ref.down_frame(0.05), s["xyz"], s["rgb"], fill_radius=3, label=label, has=has, index_base=123456)
    # -0 counts as +0: two rows of one pixel at depth +0 and -0 tie, the lower index wins and the layer holds +0
    fr = ref.frame((0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, -1), 1.0, 2, 2, -1, 1)
    pts = np.array([[0.5, -0.5, 0.0], [0.5, -0.5, -0.0]], np.float32)
    for order in ((0, 1), (1, 0)):
        got = capi.ortho_host(fr, pts[list(order)], np.zeros((2, 3), np.uint8))
        assert got["index"][0, 0] == 0 and got["depth"][0, 0].tobytes() == np.float32(0).tobytes()
    # an empty map stays empty, whatever the radius
    got = capi.ortho_host(fr, pts + 50, np.zeros((2, 3), np.uint8), fill_radius=9)
    assert got["occupied"] == 0 and got["filled"] == 0 and (got["source"] == -1).all() and (got["index"] == 0xFFFFFFFF).all()


def test_ord_is_monotone():
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32)
    f = bits.view(np.float32)
    keep = np.isfinite(f)
    f, bits = f[keep], bits[keep]
    assert (f < 0).sum() > 10000 and (f > 0).sum() > 10000
    order = np.argsort(ref.ord_bits(bits), kind="stable")
    assert (np.diff(f[order].astype(np.float64)) >= 0).all()
    z = ref.ord_bits(np.array([0x80000000, 0], np.uint32))
    assert z[0] < z[1]


def test_the_librarys_winner_follows_the_floats_order():
    """50 000 pixels with two rows each, depths drawn from all finite floats of both signs: the library's ord() decides every
    pixel as the floats' own comparison does (ties, and +0 against -0, to the lower index)"""
    from pointcloudprocessor_amd import capi

    w, h = 250, 200
    rng = np.random.default_rng(12)
    bits = rng.integers(0, 1 << 32, 2 * w * h, dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] &= np.uint32(0xBF7FFFFF)  # (no infinity, no NaN)
    bits[:40] = np.tile(np.array([0, 0x80000000, 1, 0x80000001], np.uint32), 10)  # the zeros and the smallest denormals
    bits[w * h:w * h + 40] = np.tile(np.array([0x80000000, 0, 0x80000001, 1], np.uint32), 10)
    depth = bits.view(np.float32)
    col, row = np.tile(np.arange(w * h) % w, 2), np.tile(np.arange(w * h) // w, 2)
    # looking down from the origin: depth = -z exactly, pixel (col, row) holds x in [col, col + 1), y in (-(row + 1), -row]
    xyz = np.stack([col + 0.5, -(row + 0.5), -depth], axis=1).astype(np.float32)
    fmax = float(np.finfo(np.float32).max)
    fr = ref.frame((0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, -1), 1.0, w, h, -fmax, fmax)
    got = capi.ortho_host(fr, xyz, np.zeros((2 * w * h, 3), np.uint8))
    assert got["contributors"] == 2 * w * h and got["occupied"] == w * h
    first, second = depth[:w * h].astype(np.float64), depth[w * h:].astype(np.float64)
    assert (first < 0).sum() > 10000 and (first > 0).sum() > 10000 and (first < second).sum() > 10000 and (first > second).sum() > 10000
    want_index = np.where(second < first, np.arange(w * h) + w * h, np.arange(w * h)).astype(np.uint32)
    assert np.array_equal(got["index"].ravel(), want_index)
    want_depth = np.minimum(first, second).astype(np.float32)
    want_depth = np.where(want_depth == 0, np.float32(0), want_depth)
    assert got["depth"].ravel().tobytes() == want_depth.astype(np.float32).tobytes()


def test_refusals():
    from pointcloudprocessor_amd import capi

    s = _scene()
    xyz, rgb = s["xyz"][:100], s["rgb"][:100]
    good = ref.down_frame(0.05)

    def refused(code, text=None, **change):
        fr = dict(good, **change)
        with pytest.raises(capi.PcpError) as e:
            capi.ortho_host(fr, xyz, rgb, **{k: fr.pop(k) for k in ("fill_radius", "index_base") if k in fr})
        assert e.value.code == code, str(e.value)
        if text:
            assert text in str(e.value), str(e.value)
        return str(e.value)

    refused(capi.PCP_ERR_INVALID, o=[0.0, float("nan"), 0.0])
    refused(capi.PCP_ERR_INVALID, d_max=float("inf"))
    refused(capi.PCP_ERR_INVALID, gsd=2.0)
    refused(capi.PCP_ERR_INVALID, gsd=5e-5)
    refused(capi.PCP_ERR_INVALID, d_min=3.0, d_max=3.0)
    refused(capi.PCP_ERR_INVALID, "orthonormal", n=[0.0, 0.0, 1.0])  # left-handed
    refused(capi.PCP_ERR_INVALID, "orthonormal", u=[1.002, 0.0, 0.0])
    refused(capi.PCP_ERR_INVALID, "orthonormal", u=[0.999, 0.04, 0.0])
    refused(capi.PCP_ERR_INVALID, width=0)
    refused(capi.PCP_ERR_INVALID, fill_radius=1025)
    refused(capi.PCP_ERR_INVALID, fill_radius=-1)
    refused(capi.PCP_ERR_RANGE, index_base=(1 << 32) - 100)
    refused(capi.PCP_ERR_RANGE, index_base=(1 << 63) - 1)  # (the sum with n would overflow)
    # axes within 1e-3 of orthonormal are taken as given
    capi.ortho_host(dict(good, u=[0.9995, 0.0, 0.0]), xyz, rgb)
    for w, h in ((16385, 10), (10, 20000), (16384, 4097)):
        msg = refused(capi.PCP_ERR_RANGE, "fits at gsd", width=w, height=h)
        fit = float(re.search(r"fits at gsd ([0-9.eE+-]+)", msg).group(1))
        we, he = np.ceil(w * good["gsd"] / fit), np.ceil(h * good["gsd"] / fit)
        assert we <= 16384 and he <= 16384 and we * he <= 1 << 26, msg
        assert fit < 1.01 * max(w * good["gsd"] / 16384, h * good["gsd"] / 16384, np.sqrt(w * h * good["gsd"] ** 2 / (1 << 26))), msg


def test_symbols(tmp_path):
    from pointcloudprocessor_amd import capi

    L = capi.load()
    declared = capi.declared_symbols()
    for name in NEW:
        assert name in declared and hasattr(L, name), name
    src = tmp_path / "abi.c"
    calls = "\n".join(f"  (void){s};" for s in NEW)
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  pcp_ortho_frame f;\n  (void)f;\n' + calls +
                   "\n  return PCP_ABI_VERSION == 6 && sizeof(pcp_ortho_frame) == 68 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["ortho_selftest"]
    out = subprocess.run([exe, "20000"], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "ortho_selftest.cpp")
    exe = str(tmp_path / "ortho_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe, "20000"], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


# ---- pcp_ortho_fit_frame_host ---------------------------------------------------------------------------------------------
def _tilted_plane():
    """5 000 points of an exact plane in a 3 x 2 m rectangle, tilted and shifted"""
    rng = np.random.default_rng(5)
    a, b = rng.uniform(0, 3, 5000), rng.uniform(0, 2, 5000)
    e1 = np.array([0.8, 0.6, 0.0])
    e2 = np.array([-0.6 * 0.6, 0.8 * 0.6, 0.8])
    nrm = np.cross(e1, e2)
    xyz = (np.array([2.0, -1.0, 0.5]) + a[:, None] * e1 + b[:, None] * e2).astype(np.float32)
    return xyz, nrm


def test_fit_frame_on_a_tilted_plane():
    from pointcloudprocessor_amd import capi

    xyz, nrm = _tilted_plane()
    p = xyz.astype(np.float64)
    c = p.mean(axis=0)
    cov = (p - c).T @ (p - c) / len(p)
    ev, evec = np.linalg.eigh(cov)
    n_ref, u_ref = evec[:, 0], evec[:, 2]
    u_ref = u_ref * np.sign(u_ref[np.argmax(np.abs(u_ref))])
    worst = 0.0
    for viewer, want_sign in ((None, None), (c + 3 * nrm, -1), (c - 3 * nrm, +1)):
        f = capi.ortho_fit_frame_host(xyz, 0.01, viewer=viewer)
        n, u, v = (np.array(list(x), np.float64) for x in (f.n, f.u, f.v))
        if viewer is None:
            assert n[np.argmax(np.abs(n))] < 0, "without a viewer n's largest component is negative"
        else:
            assert np.dot(viewer - np.array(list(f.o), np.float64), n) < 0, "the viewer has negative depth"
            assert np.sign(np.dot(n, nrm)) == want_sign
        worst = max(worst, np.abs(n - n_ref * np.sign(np.dot(n, n_ref))).max(), np.abs(u - u_ref).max())
        assert u[np.argmax(np.abs(u))] > 0
        assert np.abs(np.cross(u, v) - n).max() < 1e-6 and np.abs(np.cross(n, u) - v).max() < 1e-6
        fr = f.as_dict()
        ok, _, depth = ref.project(fr, xyz)
        assert ok.all(), "every row is a contributor of the returned frame"
        assert np.abs(depth).max() < 1e-4, "the origin lies on the fitted plane: the depth is the relief off it"
        # the raster is the rows' bounding rectangle in the frame's own axes plus two pixels (a pixel is 0.01 m)
        for axis, size in ((u, fr["width"]), (v, fr["height"])):
            span = np.ptp((p - c) @ axis) / 0.01
            assert span + 2 - 1e-3 <= size <= span + 3 + 1e-3, (span, size)
        assert 302 <= fr["width"] <= 306 and 202 <= fr["height"] <= 206, (fr["width"], fr["height"])
        assert fr["d_min"] < -0.0099 and fr["d_max"] > 0.0099 and fr["d_max"] - fr["d_min"] < 0.0203
        got = capi.ortho_host(fr, xyz, np.zeros_like(xyz, dtype=np.uint8))
        assert got["contributors"] == len(xyz)
    print("axes against numpy.linalg.eigh, largest component difference:", worst)
    assert worst <= 1e-4
    # has: rows without the bit do not count
    has = np.ones(len(xyz), np.uint8)
    far = xyz.copy()
    far[::2] += 100.0
    has[::2] = 0
    f = capi.ortho_fit_frame_host(far, 0.01, has=has)
    assert f.as_dict() == capi.ortho_fit_frame_host(xyz[1::2], 0.01).as_dict()


def test_fit_frame_refusals():
    from pointcloudprocessor_amd import capi

    xyz, _ = _tilted_plane()
    with pytest.raises(capi.PcpError) as e:
        capi.ortho_fit_frame_host(xyz, 1e-4)  # 30 000 x 20 000 pixels
    assert e.value.code == capi.PCP_ERR_RANGE and "fits at gsd" in str(e.value), str(e.value)
    fit = float(re.search(r"fits at gsd ([0-9.eE+-]+)", str(e.value)).group(1))
    assert 3.0 / 16384 < fit < 1.05 * np.sqrt(6.0 / (1 << 26))
    f = capi.ortho_fit_frame_host(xyz, fit)
    assert f.width <= 16384 and f.height <= 16384 and f.width * f.height <= 1 << 26
    for bad in (xyz[:2], np.full((5, 3), np.nan, np.float32)):
        with pytest.raises(capi.PcpError) as e:
            capi.ortho_fit_frame_host(bad, 0.01)
        assert e.value.code == capi.PCP_ERR_INVALID
    with pytest.raises(capi.PcpError) as e:
        capi.ortho_fit_frame_host(xyz, 2.0)
    assert e.value.code == capi.PCP_ERR_INVALID
