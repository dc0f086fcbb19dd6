"""CPU suite of the crack width maps (csrc/pcp_crack_width.hpp through pcp_crack_width_host: no context, no GPU) against the
restatement in _crack_width_ref.py: flags bits 0-3, edges, w2d2 and all 13 moments by exact equality."""
import os
import subprocess

import numpy as np
import pytest

import _crack_width_ref as ref
import _mask_edt_ref as edt_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_crack_width", "pcp_crack_width_host")
RADII = (1, 3, 7, 150)


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


@pytest.fixture(scope="module")
def images():
    """shape -> (index, xyz_cam): computed once, read-only"""
    out = {}
    for shape in edt_ref.SHAPES:
        index, xyz = ref.position_image(shape, seed=100 * shape[0] + shape[1])
        index.setflags(write=False)
        xyz.setflags(write=False)
        out[shape] = (index, xyz)
    return out


def _run(mask, index, xyz, threshold, radius):
    got = _capi().crack_width_host(mask, index, xyz, threshold, radius)
    assert got["flags"].dtype == np.uint8 and got["edges"].dtype == np.int32 and got["w2d2"].dtype == np.uint32
    assert got["moments"].dtype == np.int64 and got["moments"].shape == mask.shape + (13,) and got["edges"].shape == mask.shape + (4,)
    assert not (got["flags"] & ~np.uint8(ref.INTEGER_BITS)).any()
    return got


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", edt_ref.SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_form_equals_the_restatement(images, shape, radius):
    index, xyz = images[shape]
    few = 0
    for name, mask in ref.masks(shape, seed=shape[0] + 7 * shape[1]).items():
        if name == "bytes":
            continue
        got = _run(mask, index, xyz, 0, radius)
        flags, mom = ref.check_integers(got, mask, index, xyz, 0, radius)
        few += int((mom[:, 0] < 3).sum())
        if name == "full":  # CW1: no background, sites only
            assert (got["flags"] == ref.SITE).all() and (got["edges"] == -1).all() and not got["w2d2"].any()
    if radius == 1 and shape[0] * shape[1] > 1:
        assert few > 0  # windows with fewer than three members occur


@pytest.mark.parametrize("radius", (3, 150))
def test_threshold_127(images, radius):
    shape = (45, 70)
    index, xyz = images[shape]
    mask = edt_ref.byte_mask(shape, seed=9)
    for t in (0, 127):
        ref.check_integers(_run(mask, index, xyz, t, radius), mask, index, xyz, t, radius)
    a, b = _run(mask, index, xyz, 0, radius), _run(mask, index, xyz, 127, radius)
    assert not np.array_equal(a["flags"], b["flags"])


def test_members_exclude_far_and_non_finite_positions(images):
    shape = (45, 70)
    index, xyz = images[shape]
    member, _ = ref.members(index, xyz)
    occupied = index >= 0
    with np.errstate(invalid="ignore"):
        assert (occupied & ~member).sum() >= 2 and np.isnan(xyz[occupied]).any() and (np.abs(xyz[occupied]) >= 64).any()
    got = _run(edt_ref.corner_mask(shape), index, xyz, 0, 150)  # R = 150: every window is the whole image
    assert (got["moments"][..., 0].ravel()[:-1] == member.sum()).all() and member.sum() < occupied.sum()


def test_open_trace_on_the_border_and_the_diagonal_tie():
    capi = _capi()
    # 7 x 7, foreground but the corner (0, 0): site (3, 3) has v = (3, 3), |vx| = |vy|; the near trace walks the diagonal to
    # (0, 0): f = (1, 1), b = (0, 0), E = (1, 1); the far trace leaves the image past (6, 6): open
    mask = np.full((7, 7), 255, np.uint8)
    mask[0, 0] = 0
    index = np.full((7, 7), -1, np.int32)
    xyz = np.zeros((7, 7, 3), np.float32)
    got = capi.crack_width_host(mask, index, xyz, 0, 3)
    assert got["flags"][3, 3] & ref.NEAR and not got["flags"][3, 3] & ref.FAR
    assert got["edges"][3, 3].tolist() == [1, 1, -1, -1] and got["w2d2"][3, 3] == 0
    assert got["flags"][6, 6] & ref.CENTRE and not got["flags"][3, 3] & ref.CENTRE  # the ridge is the far corner
    assert got["flags"][0, 0] == 0
    ref.check_integers(got, mask, index, xyz, 0, 3)
    # a site on the image border whose far trace leaves at once, and a two-sided one
    mask = np.zeros((5, 9), np.uint8)
    mask[2, 0:3] = 255  # a horizontal bar touching the left border; background above and below
    mask[0:5, 6] = 255  # a vertical bar from border to border
    got = capi.crack_width_host(mask, np.full((5, 9), -1, np.int32), np.zeros((5, 9, 3), np.float32), 0, 1)
    assert got["edges"][2, 0].tolist() == [0, 3, 0, 5] and got["w2d2"][2, 0] == 4  # nearest is (0, 1): up; far: down
    assert got["edges"][0, 6].tolist() == [11, 0, 13, 0]  # nearest is (5, 0): left; far: right
    assert got["flags"][0, 6] == ref.SITE | ref.CENTRE | ref.NEAR | ref.FAR and got["w2d2"][0, 6] == 4
    ref.check_integers(got, mask, np.full((5, 9), -1, np.int32), np.zeros((5, 9, 3), np.float32), 0, 1)


@pytest.fixture(scope="module")
def deep():
    index, xyz = ref.deep_wall_image()
    mask = edt_ref.random_mask(index.shape, 0.5, seed=21)
    return index, xyz, mask


def test_prefix_sums_past_2_to_64(deep):
    """the origin-moment prefix of the 1536 x 1536 wall at 60-63 m wraps; the recentred moments are exact all the same"""
    index, xyz, mask = deep
    member, q = ref.members(index, xyz)
    assert member.all()
    assert float((q[..., 0].astype(np.float64) ** 2).sum()) > 2.0 ** 64  # (the true sum of one plane: twice what 64 bits hold)
    got = _capi().crack_width_host(mask, index, xyz, 0, 150)
    ys, xs = np.nonzero(got["flags"] & ref.SITE)
    pick = np.sort(np.random.default_rng(64).choice(len(ys), 512, replace=False))
    ys, xs = ys[pick], xs[pick]
    assert np.array_equal(got["moments"][ys, xs], ref.moments_at(member, q, ys, xs, 150))
    assert got["moments"][ys, xs, 0].max() == 300 * 300


def test_error_returns():
    capi = _capi()
    mask = np.zeros((4, 6), np.uint8)
    index = np.full((4, 6), -1, np.int32)
    xyz = np.zeros((4, 6, 3), np.float32)
    for t, r in ((-1, 150), (256, 150), (0, 0), (0, 182), (0, -3)):
        with pytest.raises(capi.PcpError) as e:
            capi.crack_width_host(mask, index, xyz, t, r)
        assert e.value.code == capi.PCP_ERR_INVALID, (t, r)
    assert capi.crack_width_host(mask, index, xyz, 255, 181)["flags"].shape == (4, 6)
    lib, C = capi.load(), capi.C
    prm = capi.CrackParams(0, 150)
    args = (C.c_int32(6), C.c_int32(4), capi._ptr(mask), C.c_int64(6), capi._ptr(index), capi._ptr(xyz))
    assert lib.pcp_crack_width_host(*args, None, None, None, None, None) == capi.PCP_ERR_INVALID  # NULL params
    assert lib.pcp_crack_width_host(C.c_int32(6), C.c_int32(4), None, C.c_int64(6), capi._ptr(index), capi._ptr(xyz), C.byref(prm),
                                    None, None, None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_crack_width_host(C.c_int32(6), C.c_int32(4), capi._ptr(mask), C.c_int64(5), capi._ptr(index), capi._ptr(xyz),
                                    C.byref(prm), None, None, None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_crack_width_host(C.c_int32(16385), C.c_int32(1), capi._ptr(mask), C.c_int64(16385), capi._ptr(index), capi._ptr(xyz),
                                    C.byref(prm), None, None, None, None) == capi.PCP_ERR_RANGE
    assert lib.pcp_crack_width_host(C.c_int32(16384), C.c_int32(4097), capi._ptr(mask), C.c_int64(16384), capi._ptr(index),
                                    capi._ptr(xyz), C.byref(prm), None, None, None, None) == capi.PCP_ERR_RANGE  # W * H > 2^26
    assert b"16384" in lib.pcp_last_error(None)
    assert lib.pcp_crack_width_host(*args, C.byref(prm), None, None, None, None) == capi.PCP_OK  # every output nullable
    assert lib.pcp_crack_width(None, C.c_int32(0), C.byref(prm), None, None, None, None, None, None, None, None, None) == capi.PCP_ERR_INVALID


def test_header_constants():
    text = open(os.path.join(ROOT, "pointcloudprocessor_amd", "csrc", "pcp_crack_width.hpp")).read()
    for line in ("kSite = 1, kCentre = 2, kNear = 4, kFar = 8, kPlane = 16, kRays = 32, kWidth = 64", "kMinRadius = 1, kMaxRadius = 181",
                 "kQuantaPerMetre = 65536.0f", "kMaxCoordinate = 64.0f", "kMomentWords = 13", "kUndistortSteps = 10",
                 "kReprojectionPx = 1e-3", "kMinIncidence = 0.1"):
        assert line in text, line
    capi = _capi()
    assert (capi.CW_SITE, capi.CW_CENTRE, capi.CW_NEAR, capi.CW_FAR, capi.CW_PLANE, capi.CW_RAYS, capi.CW_WIDTH) == (
        ref.SITE, ref.CENTRE, ref.NEAR, ref.FAR, ref.PLANE, ref.RAYS, ref.WIDTH)


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    assert callable(capi.Context.crack_width) and callable(capi.crack_width_host)
    assert lib.pcp_abi_version() == 6 and capi.K_COUNT == 13
    assert capi.C.sizeof(capi.CrackParams) == 8


def test_header_with_the_new_declarations_is_plain_c(tmp_path):
    src = tmp_path / "abi.c"
    calls = "\n".join(f"  (void){s};" for s in NEW)
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  pcp_crack_params p = {0, 150};\n  (void)p;\n' + calls +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && sizeof(pcp_crack_params) == 8 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["crack_width_selftest"]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "crack_width_selftest.cpp")
    exe = str(tmp_path / "crack_width_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe, "300"], capture_output=True, text=True)  # (the default size, whose tables wrap, runs unsanitised above)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_pipeline_refuses_index_shards():
    from pointcloudprocessor_amd import pipeline

    with pytest.raises(ValueError) as e:
        pipeline.PointCloudColorizer(None, rank=0, world=2).crack_width(0)
    assert "index shard" in str(e.value) and "not built" in str(e.value)
