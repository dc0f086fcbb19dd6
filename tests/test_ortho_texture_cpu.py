"""The orthophoto's surface points without a GPU ("Orthophotos", OT2, OT3, OT9): pcp_ortho_texture_points_host against
the restatement in _ortho_texture_ref.py on the base scene's map (test_ortho_gpu.py's: 242 x 202 pixels at gsd 0.05, filled at
R = 2), the refusals, the symbols, and the stand-alone selftest plain and under the host sanitizers.  Every comparison is exact
equality of the bytes."""
import os
import subprocess

import numpy as np
import pytest

import _ortho_ref as oref
import _ortho_texture_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECT = (37, 21, 50, 40)  # ortho pixels: inside the room, not the whole raster


@pytest.fixture(scope="module")
def base_map():
    from pointcloudprocessor_amd import capi

    s = oref.base_scene()
    fr = oref.down_frame(0.05)
    m = capi.ortho_host(fr, s["xyz"], s["rgb"], fill_radius=2)
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    assert (fr["width"], fr["height"]) == (242, 202) and m["occupied"] >= 10000 and m["filled"] >= 30000
    return fr, m


def test_the_symbols_are_exported():
    from pointcloudprocessor_amd import capi

    lib = capi.load()
    assert hasattr(lib, "pcp_ortho_texture") and hasattr(lib, "pcp_ortho_texture_points_host")
    assert {"pcp_ortho_texture", "pcp_ortho_texture_points_host"} <= set(capi.declared_symbols())


@pytest.mark.parametrize("k", [1, 2, 3, 4, 16])
def test_host_points_equal_the_restatement(base_map, k):
    from pointcloudprocessor_amd import capi

    fr, m = base_map
    results = {}
    for interpolate in (False, True):
        for max_step in (0.05, 100.0):  # 0.05 cuts the steps between floor, furniture and walls; 100 cuts nothing
            ok, xyz = ref.surface(fr, m["source"], m["depth"], k, interpolate, max_step, RECT)
            got = capi.ortho_texture_points_host(fr, m["source"], m["depth"], k, interpolate, max_step, RECT)
            assert got["ok"].shape == (RECT[3] * k, RECT[2] * k) and got["xyz"].shape == got["ok"].shape + (3,)
            assert got["ok"].tobytes() == ok.astype(np.uint8).tobytes()
            assert got["xyz"].tobytes() == xyz.tobytes(), (k, interpolate, max_step)
            results[interpolate, max_step] = xyz
    n = int(ok.sum())
    off, cut, free = results[False, 0.05], results[True, 0.05], results[True, 100.0]
    assert results[False, 100.0].tobytes() == off.tobytes()
    moved_cut = int((cut != off).any(axis=2).sum())
    moved_free = int((free != off).any(axis=2).sum())
    print(f"k {k}: {n} surface pixels of {ok.size}, moved by the interpolation: {moved_cut} at 0.05, {moved_free} at 100")
    assert n >= 1000 * k * k and n < ok.size, "the rectangle holds surface and holes"
    if k == 1:
        assert moved_cut == 0 and moved_free == 0, "at k = 1 every fine pixel is a centre"
    else:
        assert 0 < moved_cut < moved_free, "the smaller step cuts some neighbours, the larger none of them"


def test_four_rectangles_make_the_whole(base_map):
    from pointcloudprocessor_amd import capi

    fr, m = base_map
    k = 3
    W, H = fr["width"], fr["height"]
    whole = capi.ortho_texture_points_host(fr, m["source"], m["depth"], k, True, 0.05)
    ok, xyz = ref.surface(fr, m["source"], m["depth"], k, True, 0.05)
    assert whole["xyz"].tobytes() == xyz.tobytes() and whole["ok"].tobytes() == ok.astype(np.uint8).tobytes()
    cx, cy = 101, 77  # (odd cuts: the rectangles' borders are interior to the interpolation)
    parts = [capi.ortho_texture_points_host(fr, m["source"], m["depth"], k, True, 0.05, rect)
             for rect in ((0, 0, cx, cy), (cx, 0, W - cx, cy), (0, cy, cx, H - cy), (cx, cy, W - cx, H - cy))]
    for key in ("xyz", "ok"):
        joined = np.concatenate([np.concatenate([parts[0][key], parts[1][key]], axis=1),
                                 np.concatenate([parts[2][key], parts[3][key]], axis=1)], axis=0)
        assert joined.tobytes() == whole[key].tobytes(), key


def test_refusals(base_map):
    from pointcloudprocessor_amd import capi

    fr, m = base_map
    W, H = fr["width"], fr["height"]

    def call(scale=2, interpolate=True, max_step=0.05, rect=None, frame=fr, views=1):
        f = capi.ortho_frame(frame)
        p = capi.ortho_texture_params(scale, views, interpolate, max_step, rect)
        src = np.ascontiguousarray(m["source"] if frame is fr else np.zeros((frame["height"], frame["width"]), np.int32))
        dep = np.ascontiguousarray(m["depth"] if frame is fr else np.zeros((frame["height"], frame["width"]), np.float32))
        one = np.zeros(16, np.float32)  # (a refused call writes nothing)
        rc = capi.load().pcp_ortho_texture_points_host(capi.C.byref(f), capi.C.byref(p), capi._ptr(src), capi._ptr(dep), capi._ptr(one), None)
        return rc, capi.load().pcp_last_error(None).decode()

    invalid = [dict(scale=0), dict(scale=17), dict(scale=-3), dict(views=0), dict(views=6), dict(rect=(0, 0, 10, 0)), dict(rect=(0, 0, 0, 10)),
               dict(rect=(W - 9, 0, 10, 10)), dict(rect=(0, H - 9, 10, 10)), dict(rect=(-1, 0, 10, 10)), dict(rect=(0, -1, 10, 10)),
               dict(rect=(0, 0, W + 1, H)), dict(rect=(0, 0, -5, -5)), dict(rect=(3, 0, 0, 0)), dict(max_step=0.0), dict(max_step=-0.05),
               dict(max_step=float("inf")), dict(max_step=float("nan"))]
    for kw in invalid:
        rc, msg = call(**kw)
        assert rc == capi.PCP_ERR_INVALID, (kw, rc, msg)
        assert "pcp_ortho_texture_points_host" in msg
    # the limit of 2^28 fine pixels: the message names the largest scale that fits the rectangle
    big = oref.frame((0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, -1), 0.01, 8192, 4096, 0.0, 1.0)
    rc, msg = call(scale=3, frame=big)
    assert rc == capi.PCP_ERR_RANGE and "largest scale that fits the rectangle is 2" in msg, msg
    rc, msg = call(scale=16, frame=big, rect=(100, 100, 2048, 1024))
    assert rc == capi.PCP_ERR_RANGE and "is 11" in msg, msg  # 2^21 pixels: k * k <= 128
    # the frame's own rules come first
    rc, msg = call(frame=dict(fr, gsd=2.0))
    assert rc == capi.PCP_ERR_INVALID
    # NULL arguments
    L = capi.load()
    f, p = capi.ortho_frame(fr), capi.ortho_texture_params(2)
    assert L.pcp_ortho_texture_points_host(None, capi.C.byref(p), capi._ptr(m["source"]), capi._ptr(m["depth"]), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_ortho_texture_points_host(capi.C.byref(f), None, capi._ptr(m["source"]), capi._ptr(m["depth"]), None, None) == capi.PCP_ERR_INVALID
    assert L.pcp_ortho_texture_points_host(capi.C.byref(f), capi.C.byref(p), None, capi._ptr(m["depth"]), None, None) == capi.PCP_ERR_INVALID
    # a source image that names a pixel outside the map
    bad = m["source"].copy()
    bad[5, 5] = W * H
    with pytest.raises(capi.PcpError) as e:
        capi.ortho_texture_points_host(fr, bad, m["depth"], 2)
    assert e.value.code == capi.PCP_ERR_INVALID
    # the wrapper's own refusal of layers of another shape
    with pytest.raises(ValueError):
        capi.ortho_texture_points_host(fr, m["source"][:-1], m["depth"][:-1], 2)
    # both outputs are nullable
    assert L.pcp_ortho_texture_points_host(capi.C.byref(f), capi.C.byref(p), capi._ptr(np.ascontiguousarray(m["source"])),
                                           capi._ptr(np.ascontiguousarray(m["depth"])), None, None) == capi.PCP_OK


def _checksum(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("checksum ")]
    assert len(lines) == 1, out
    return lines[0]


def test_selftest_plain_and_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own: the project's build of it, and one with the address and
    undefined-behaviour sanitizers, on the CPU; both print the same checksum over every bit OT3 produces."""
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["ortho_texture_selftest"]
    plain = subprocess.run([exe], capture_output=True, text=True)
    assert plain.returncode == 0 and "0 mismatches" in plain.stdout, plain.stdout + plain.stderr
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "ortho_texture_selftest.cpp")
    san_exe = str(tmp_path / "ortho_texture_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", san_exe], check=True, capture_output=True)
    san = subprocess.run([san_exe], capture_output=True, text=True)
    assert san.returncode == 0 and "0 mismatches" in san.stdout, san.stdout + san.stderr
    assert _checksum(san.stdout) == _checksum(plain.stdout)
