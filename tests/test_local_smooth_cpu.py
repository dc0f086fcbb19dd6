"""smoothColorsWithLocalRegion without a GPU: the restatement against exact rational arithmetic,
known answers for each rule, the C ABI / Python surface and the command line's parse-time rejection of bad radii."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _local_smooth_ref as ref


def _cloud(rng, n, extent=0.3):
    x, y, z = (rng.uniform(0.0, extent, n).astype(np.float32) for _ in range(3))
    w = rng.integers(0, 1 << 24, n, dtype=np.uint32)
    w[rng.random(n) < 0.2] = 0  # never-seen points
    return x, y, z, w


@pytest.mark.parametrize("seed,n,radius", [(0, 40, 0.1), (1, 120, 0.05), (2, 300, 0.08), (3, 200, 1.0)])
def test_restatement_equals_rational_brute_force(seed, n, radius):
    rng = np.random.default_rng(seed)
    x, y, z, w = _cloud(rng, n)
    if seed == 2:  # duplicates and non-finite points
        x[5], y[5], z[5] = x[6], y[6], z[6]
        x[7] = np.nan
        z[8] = np.inf
    got = ref.smooth_local(x, y, z, w, radius)
    want = ref.brute_force_fraction(x, y, z, w, radius)
    assert np.array_equal(got, want)


def test_lone_point_keeps_its_colour():
    x, y, z = (np.array([v], np.float32) for v in (1.0, 2.0, 3.0))
    for word in (0x00123456, 0x01123456, 0):
        out = ref.smooth_local(x, y, z, np.array([word], np.uint32), 0.1)
        want = ref.pack(word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF)
        assert out[0] == want


def _threshold(r):
    r2 = float(np.float32(r)) ** 2
    t = np.float32(r2)
    if float(t) > r2:
        t = np.nextafter(t, np.float32(0))
    return t


def test_ls2_boundary_exactly_on_t_and_one_ulp_above():
    r = np.float32(0.1)
    t = _threshold(r)
    # a pair along x whose fp32 squared distance is exactly t, and the next float above: find dx with fl32(dx*dx) == t
    dx = np.float32(np.sqrt(np.float64(t)))
    for _ in range(64):
        if np.float32(dx * dx) <= t:
            break
        dx = np.nextafter(dx, np.float32(0))
    while np.float32(np.nextafter(dx, np.float32(1)) ** 2) <= t:
        dx = np.nextafter(dx, np.float32(1))
    assert np.float32(dx * dx) <= t
    x0 = np.float32(0.0)
    inside = np.array([x0, dx], np.float32)
    d2 = np.float32(inside[1] - inside[0]) ** 2
    assert np.float32(d2) <= t and float(np.float32(d2)) <= float(r) * float(r)
    dx_out = np.nextafter(dx, np.float32(1))
    assert np.float32(dx_out * dx_out) > t
    zeros = np.zeros(2, np.float32)
    words = np.array([ref.pack(200, 0, 0), ref.pack(0, 0, 100)], np.uint32)
    got_in = ref.smooth_local(inside, zeros, zeros, words, r)
    got_out = ref.smooth_local(np.array([x0, dx_out], np.float32), zeros, zeros, words, r)
    assert np.array_equal(got_out, words)  # one ulp above t: each point alone
    # inside: point 0 takes w = 1 on itself and w(d2) on point 1
    w = np.float32(1) / np.float32(np.float32(1) + np.float32(dx * dx))
    m = int(np.float64(w) * 16777216.0)
    S = 16777216 + m
    assert got_in[0] == ref.pack(200 * 16777216 // S, 0, 100 * m // S)
    assert got_in[1] == ref.pack(200 * m // S, 0, 100 * 16777216 // S)
    # the rule compares in fp64: t itself is inside, and t is the largest such float
    assert float(t) <= float(r) * float(r) < float(np.nextafter(t, np.float32(1)))


def test_uniform_patch_keeps_exactly_its_colour():
    rng = np.random.default_rng(5)
    x, y, z, _ = _cloud(rng, 500, 0.2)
    w = np.full(500, ref.pack(17, 130, 251), np.uint32)
    assert np.array_equal(ref.smooth_local(x, y, z, w, 0.05), w)


def test_never_seen_point_between_coloured_ones_gets_a_colour():
    x = np.array([0.0, 0.01, 0.02], np.float32)
    zeros = np.zeros(3, np.float32)
    words = np.array([ref.pack(90, 90, 90), 0, ref.pack(90, 90, 90)], np.uint32)
    out = ref.smooth_local(x, zeros, zeros, words, 0.1)
    assert (words[1] >> 24) == 0 and (out[1] >> 24) == 1
    # floor of a mean of 0 and 90s: between 0 and 90, the two end points lose a little to their black neighbour
    r = int(out[1] & 0xFF)
    assert 0 < r < 90


def test_nan_points_are_left_alone_and_take_no_part():
    x = np.array([0.0, np.nan, 0.01, 0.0], np.float32)
    y = np.array([0.0, 0.0, 0.0, np.inf], np.float32)
    z = np.zeros(4, np.float32)
    words = np.array([ref.pack(10, 0, 0), ref.pack(250, 250, 250) | (1 << 24), ref.pack(10, 0, 0), 0x00ABCDEF], np.uint32)
    out = ref.smooth_local(x, y, z, words, 0.1)
    assert out[1] == words[1] and out[3] == words[3]
    assert out[0] == ref.pack(10, 0, 0) and out[2] == ref.pack(10, 0, 0)


def test_bad_radius_is_rejected_by_the_restatement():
    one = np.zeros(1, np.float32)
    for r in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ref.smooth_local(one, one, one, np.zeros(1, np.uint32), r)


def test_header_declares_and_library_exports_the_entry_points():
    from pointcloudprocessor_amd import _build, capi

    syms = capi.declared_symbols()
    assert "pcp_colour_smooth_local" in syms and "pcp_colour_smooth_local_packed" in syms
    _build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB_PATH], capture_output=True, text=True).stdout
    for s in ("pcp_colour_smooth_local", "pcp_colour_smooth_local_packed"):
        assert re.search(rf"\bT {s}$", out, re.M), s
    with open(os.path.join(_build.INCLUDE, "pcp_hip.h")) as f:
        text = f.read()
    assert re.search(r"PCP_K_COLOUR_SMOOTH\s*=\s*12", text) and re.search(r"PCP_K_COUNT\s*=\s*13", text)


def test_kernel_ids_and_names():
    from pointcloudprocessor_amd import capi

    assert capi.K_COLOUR_SMOOTH == 12 and capi.K_COUNT == 13
    lib = capi.load()
    names = [lib.pcp_kernel_name(k).decode() for k in range(capi.K_COUNT)]
    assert len(set(names)) == capi.K_COUNT and "?" not in names
    assert names[capi.K_COLOUR_SMOOTH] == "colour_smooth"
    assert lib.pcp_kernel_name(capi.K_COUNT).decode() == "?"


def test_pipeline_refuses_the_sharded_form():
    from pointcloudprocessor_amd.pipeline import PointCloudColorizer

    with pytest.raises(ValueError):
        PointCloudColorizer(engine=None, rank=0, world=2).run(local_smooth_radius=0.1)


@pytest.mark.parametrize("value", ["-1", "nan", "2", "x"])
def test_cli_rejects_bad_radius_before_any_device_use(tmp_path, value):
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    exe = host_build.build()["PointCloudProcessor"]
    # the input files do not exist: a radius that passed the parser would fail later, on reading the cloud
    p = subprocess.run([exe, "--smoothColorsRadius", value, "-p", str(tmp_path / "none.pcd"), "-o", str(tmp_path / "odo.txt"),
                        "-i", str(tmp_path) + "/"], capture_output=True, text=True)
    assert p.returncode == 254
    assert f"the argument ('{value}') for option '--smoothColorsRadius' is invalid" in p.stderr
    assert "Couldn't read point cloud file." not in p.stderr
    assert not os.path.exists(tmp_path / "cloudInWorldWithRGB.pcd")


def test_exact_integer_weights_reproduce_rational_weights():
    # LS4: with r <= 1 every w lies in [0.5, 1] and w * 2^24 is an integer
    for d2 in np.float32([0.0, 1e-8, 0.0025, 0.01, 0.5, 1.0]):
        w = np.float32(1) / np.float32(np.float32(1) + d2)
        assert 0.5 <= w <= 1.0
        assert Fraction(float(w)) * 2 ** 24 == int(np.float64(w) * 16777216.0)
