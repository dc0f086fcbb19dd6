"""The keyframe colour balance without a GPU ("Image balance"): pcp_image_balance_host against the numpy
restatement in _image_balance_ref.py on every shape, image and parameter the GPU tests use (histograms, tables and pixels, all
exactly equal), the gamma table, the refusals, the ABI, and the stand-alone selftest plain and under the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import _image_balance_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pcp_default_balance_params", "pcp_set_image_balance", "pcp_image_balance", "pcp_image_balance_host", "pcp_gamma_table_host"]


def _same(capi, im, **p):
    want = ref.balance(im, **p)
    got = capi.image_balance_host(im, p, stages=True)
    assert np.array_equal(got["bgr"], want["bgr"]), ("pixels", p, int((got["bgr"] != want["bgr"]).sum()))
    if p["stages"] & 1:
        assert np.array_equal(got["hist"], want["hist"]), ("hist", p)
        assert np.array_equal(got["lut"], want["lut"]), ("lut", p)
        assert got["hist"].sum(axis=2).min() == got["hist"].sum(axis=2).max(), "every tile counts its tw * th extended pixels"
    else:
        assert "hist" not in got and "lut" not in got
    return want


@pytest.mark.parametrize("kind", ref.IMAGES)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_t{s[2]}x{s[3]}")
def test_host_equals_the_restatement(shape, kind):
    from pointcloudprocessor_amd import capi

    w, h, tx, ty = shape
    im = ref.image(kind, w, h)
    im.setflags(write=False)
    for clip in ref.CLIPS:
        for gamma in ref.GAMMAS:
            _same(capi, im, stages=3, tiles=(tx, ty), clip_limit=clip, gamma=gamma)
    _same(capi, im, stages=1, tiles=(tx, ty), clip_limit=3.0, gamma=0.8)
    _same(capi, im, stages=2, tiles=(tx, ty), clip_limit=1.0, gamma=1.1)


def test_host_at_1080p_with_the_defaults():
    from pointcloudprocessor_amd import capi

    im = ref.looks_real(1920, 1080)
    want = _same(capi, im, stages=3, tiles=(8, 8), clip_limit=1.0, gamma=0.8)
    assert np.array_equal(capi.image_balance_host(im), want["bgr"]), "the defaults are the autonomous script's main()"
    assert (want["bgr"] != im).mean() > 0.5


def test_what_the_shapes_are_there_for():
    """the cases exercise what their comments say"""
    assert ref.grid(64, 48, 8, 8) == (0, 0, 8, 6) and max(int(1.0 * 48 / 256), 1) == 1
    assert ref.grid(70, 50, 8, 8) == (2, 6, 9, 7)
    assert ref.grid(64, 50, 8, 8) == (8, 6, 9, 7), "a side that divides evenly is extended by a whole tile count"
    assert ref.grid(48, 36, 1, 1) == (0, 0, 48, 36)
    assert ref.grid(512, 384, 2, 2)[2:] == (256, 192)
    # the constant image: one bin holds the tile; the residual walk runs with step > 1
    total, clip = 48, 1
    clipped = total - clip
    assert 0 < clipped % 256 < 128 and 256 // (clipped % 256) > 1
    # halves of the HSV round trip: the restatement's own agree with the oracle's whole
    assert ref.hsv_halves_agree_with_the_oracle(ref.image("noise", 64, 48))
    v = np.arange(0, 256, 5, dtype=np.uint8)
    lattice = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 1, 3)
    assert ref.hsv_halves_agree_with_the_oracle(lattice)


def test_gamma_table():
    from pointcloudprocessor_amd import capi

    for g in ref.GAMMAS:
        want = np.array([((i / 255.0) ** (1.0 / float(np.float32(g)))) * 255.0 for i in range(256)])
        assert np.array_equal(capi.gamma_table_host(g), want.astype(np.uint8)), g
        if g != 1.0:  # no entry close enough to an integer for the libm in use to matter, with gamma as a float or a double
            frac = np.minimum(want - np.floor(want), np.ceil(want) - want)[1:255]
            assert frac.min() > 5e-4, (g, frac.min())
            assert np.array_equal(want.astype(np.uint8), np.array([((i / 255.0) ** (1.0 / g)) * 255.0 for i in range(256)]).astype(np.uint8))
    assert np.array_equal(capi.gamma_table_host(1.0), np.arange(256, dtype=np.uint8))


def test_refusals():
    from pointcloudprocessor_amd import capi

    im = ref.image("noise", 64, 48)

    def refused(code, image=im, **p):
        with pytest.raises(capi.PcpError) as e:
            capi.image_balance_host(image, p)
        assert e.value.code == code, str(e.value)

    refused(capi.PCP_ERR_INVALID, tiles=(0, 8))
    refused(capi.PCP_ERR_INVALID, tiles=(8, 17))
    refused(capi.PCP_ERR_INVALID, tiles=(17, 8), stages=2)
    refused(capi.PCP_ERR_INVALID, gamma=0.0)
    refused(capi.PCP_ERR_INVALID, gamma=-1.0)
    refused(capi.PCP_ERR_INVALID, gamma=float("nan"))
    refused(capi.PCP_ERR_INVALID, gamma=float("inf"))
    refused(capi.PCP_ERR_INVALID, clip_limit=float("nan"))
    refused(capi.PCP_ERR_INVALID, stages=4)
    for g in (0.0, -2.0, float("nan")):
        with pytest.raises(capi.PcpError) as e:
            capi.gamma_table_host(g)
        assert e.value.code == capi.PCP_ERR_INVALID
    # IB3: the extension must stay below the side, so that every reflected index 2 (n - 1) - i lies in the image
    refused(capi.PCP_ERR_RANGE, image=ref.image("noise", 8, 9), tiles=(8, 8))    # 8 divides: extended by a whole 8 >= 8
    refused(capi.PCP_ERR_RANGE, image=ref.image("noise", 4, 4), tiles=(8, 8))
    refused(capi.PCP_ERR_RANGE, image=ref.image("noise", 20, 8), tiles=(16, 16))
    capi.image_balance_host(ref.image("noise", 8, 9), dict(tiles=(8, 8), stages=2))  # the gamma stage alone has no grid


def test_9x9_with_8x8_tiles():
    """The issue lists this case among the refusals ("the extension reaches past the image") and also defines the refusal as
    extension >= w or >= h.  Here the extension is 8 - 9 % 8 = 7 < 9: the extended side is 16, and the furthest reflected index
    is 2 * 8 - 15 = 1, inside the image.  The rule is the definition (IB3), so the case is computed, and it must equal the
    restatement, whose np.pad(mode="reflect") would raise if the pad reached past the image."""
    from pointcloudprocessor_amd import capi

    assert ref.grid(9, 9, 8, 8) == (7, 7, 2, 2)
    for kind in ref.IMAGES:
        _same(capi, ref.image(kind, 9, 9), stages=3, tiles=(8, 8), clip_limit=1.0, gamma=0.8)


def test_symbols_and_abi(tmp_path):
    from pointcloudprocessor_amd import capi

    L = capi.load()
    declared = capi.declared_symbols()
    for name in NEW:
        assert name in declared and hasattr(L, name), name
    assert C_sizeof(capi.BalanceParams) == 20
    p = capi.balance_params()
    assert (p.stages, p.tiles_x, p.tiles_y, p.clip_limit, round(p.gamma, 6)) == (3, 8, 8, 1.0, 0.8)
    src = tmp_path / "abi.c"
    calls = "\n".join(f"  (void){s};" for s in NEW)
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  pcp_balance_params p;\n  (void)p;\n' + calls +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && sizeof(pcp_balance_params) == 20 && PCP_BALANCE_CLAHE == 1 &&"
                   " PCP_BALANCE_GAMMA == 2 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)
    check = tmp_path / "size.c"
    check.write_text('#include "pcp_hip.h"\ntypedef char size_is_20[sizeof(pcp_balance_params) == 20 ? 1 : -1];\n'
                     "typedef char version_is_6[PCP_ABI_VERSION == 6 ? 1 : -1];\ntypedef char count_is_13[PCP_K_COUNT == 13 ? 1 : -1];\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(check), "-c", "-o", exe + ".o"],
                   check=True, capture_output=True)
    assert capi.K_COUNT == 13


def C_sizeof(t):
    import ctypes

    return ctypes.sizeof(t)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["image_balance_selftest"]
    out = subprocess.run([exe, "1"], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "image_balance_selftest.cpp")
    exe = str(tmp_path / "image_balance_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe, "1"], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout + out.stderr
