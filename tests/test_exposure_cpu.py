"""Exposure gains, the part that needs no GPU: pcp_exposure_gains against known answers and the numpy restatement
(_exposure_ref.py), the restatement's finalise against the oracle, the equalisation property on the oracle's lists, the new
ABI surface, the CLI's flag checks and the cross-compiled kernels' resource notes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _exposure_ref as ex
from conftest import cam_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _capi():
    from pointcloudprocessor_amd import _build, capi

    _build.build()
    capi.load()
    return capi


def _random_stats(rng, F, fill=0.6, empty_rows=()):
    """symmetric n, sums with a per-keyframe brightness so that the means are consistent"""
    k = rng.uniform(0.6, 1.5, F)
    n = np.zeros((F, F), np.uint64)
    s = np.zeros((F, F), np.uint64)
    for i in range(F):
        for j in range(i + 1, F):
            if i in empty_rows or j in empty_rows or rng.random() > fill:
                continue
            c = int(rng.integers(1, 5000))
            base = rng.uniform(40, 150)
            n[i, j] = n[j, i] = c
            s[i, j] = int(min(247.0, base * k[i]) * c)
            s[j, i] = int(min(247.0, base * k[j]) * c)
    return n, s


def test_equal_means_give_unit_gains():
    capi = _capi()
    F = 5
    n = np.full((F, F), 37, np.uint64)
    np.fill_diagonal(n, 0)
    g = capi.exposure_gains(n, n * np.uint64(100))
    assert np.all(np.abs(g - 1.0) <= 1e-12), g


def test_a_keyframe_without_pairs_gets_exactly_one():
    capi = _capi()
    rng = np.random.default_rng(3)
    n, s = _random_stats(rng, 6, fill=1.0, empty_rows=(2,))
    g = capi.exposure_gains(n, s)
    assert g[2] == 1.0
    assert np.all(g[[0, 1, 3, 4, 5]] != 1.0)
    # no pair at all: every gain is exactly one
    z = np.zeros((4, 4), np.uint64)
    assert np.array_equal(capi.exposure_gains(z, z), np.ones(4))
    assert np.array_equal(capi.exposure_gains(np.zeros((1, 1), np.uint64), np.zeros((1, 1), np.uint64)), np.ones(1))


@pytest.mark.parametrize("a,b,N,sn,sg", [(100.0, 140.0, 1000, 10.0, 0.1), (60.0, 200.0, 7, 5.0, 0.3), (128.0, 128.0, 3, 10.0, 0.1)])
def test_two_keyframes_closed_form(a, b, N, sn, sg):
    capi = _capi()
    n = np.array([[0, N], [N, 0]], np.uint64)
    s = np.array([[0, int(a * N)], [int(b * N), 0]], np.uint64)
    p, q, r, w = a * a / sn**2, b * b / sn**2, a * b / sn**2, 1.0 / sg**2
    det = (p + w) * (q + w) - r * r
    want = np.array([w * (q + w + r) / det, w * (p + w + r) / det])
    g = capi.exposure_gains(n, s, sn, sg)
    assert np.allclose(g, want, rtol=1e-12, atol=0.0), (g, want)
    assert (g[0] > g[1]) == (a < b) or a == b


@pytest.mark.parametrize("F,seed", [(7, 11), (33, 12)])
def test_random_systems_match_the_restatement(F, seed):
    capi = _capi()
    rng = np.random.default_rng(seed)
    n, s = _random_stats(rng, F, empty_rows=(1,) if F == 7 else (4, 20))
    for sn, sg in ((10.0, 0.1), (4.0, 0.5)):
        g = capi.exposure_gains(n, s, sn, sg)
        want = ex.gains(n, s, sn, sg)
        assert np.max(np.abs(g - want) / np.abs(want)) <= 1e-10
        assert np.array_equal(g == 1.0, want == 1.0)
    # deterministic: the same bits on every call
    assert np.array_equal(capi.exposure_gains(n, s), capi.exposure_gains(n, s))


def test_refused_arguments():
    capi = _capi()
    lib = capi.load()
    n = np.array([[0, 5], [5, 0]], np.uint64)
    s = np.array([[0, 500], [600, 0]], np.uint64)
    assert capi.exposure_gains(n, s).shape == (2,)

    def code(fn):
        with pytest.raises(capi.PcpError) as e:
            fn()
        return e.value.code

    for sn, sg in ((0.0, 0.1), (-1.0, 0.1), (np.nan, 0.1), (np.inf, 0.1), (10.0, 0.0), (10.0, -0.1), (10.0, np.nan), (10.0, np.inf)):
        assert code(lambda: capi.exposure_gains(n, s, sn, sg)) == capi.PCP_ERR_INVALID, (sn, sg)
    asym = n.copy()
    asym[0, 1] = 6
    assert code(lambda: capi.exposure_gains(asym, s)) == capi.PCP_ERR_INVALID
    big = s.copy()
    big[1, 0] = 255 * 5 + 1
    assert code(lambda: capi.exposure_gains(n, big)) == capi.PCP_ERR_INVALID
    big[1, 0] = 255 * 5
    capi.exposure_gains(n, big)
    out = np.zeros(2)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fn = lib.pcp_exposure_gains
    assert fn(C.c_int32(0), p(n), p(s), C.c_double(10), C.c_double(0.1), p(out)) == capi.PCP_ERR_INVALID
    assert fn(C.c_int32(-3), p(n), p(s), C.c_double(10), C.c_double(0.1), p(out)) == capi.PCP_ERR_INVALID
    assert fn(C.c_int32(2), None, p(s), C.c_double(10), C.c_double(0.1), p(out)) == capi.PCP_ERR_INVALID
    # more keyframes than the dense solve is built for: refused before the matrices are read
    assert fn(C.c_int32(4097), p(n), p(s), C.c_double(10), C.c_double(0.1), p(out)) == capi.PCP_ERR_RANGE
    assert b"4097" in lib.pcp_last_error(None)


@pytest.fixture(scope="module")
def oracle_lists(oracle, small_scene):
    sc = small_scene
    return oracle.colorize(cam_struct(oracle, sc["cam"]), oracle.default_cull_params(), sc["x"], sc["y"], sc["z"], sc["poses"], sc["images"])


def test_restated_finalise_with_unit_gains_is_the_oracle(oracle_lists):
    ref = oracle_lists
    rgb, has = ex.finalise(ref["top_score"], ref["top_rgb"], ref["top_frame"], np.ones(6))
    seen = ref["top_frame"][:, 0] >= 0
    assert seen.sum() > 1000
    assert np.array_equal(rgb[seen], ref["rgb"][seen]) and np.array_equal(has, ref["has"])
    assert not rgb[~seen].any()


def test_gains_equalise_keyframes_of_different_exposure(oracle, small_scene):
    """small_scene's geometry under uniform grey keyframes of brightness 128 k_f: the gains pull the keyframes together --
    the spread of log(g_f k_f) is at most half that of log(k_f) (the prior sigma_g stops short of full equalisation; the
    restatement alone measures 0.35)."""
    capi = _capi()
    sc = small_scene
    ref = oracle.colorize(cam_struct(oracle, sc["cam"]), oracle.default_cull_params(), sc["x"], sc["y"], sc["z"], sc["poses"],
                          ex.grey_images(sc["cam"]))
    n, s = ex.pair_stats(ref["top_frame"], ref["top_rgb"], 6)
    assert np.array_equal(n, n.T) and (n > 0).sum() >= 20
    g = capi.exposure_gains(n, s)
    assert np.max(np.abs(g - ex.gains(n, s)) / ex.gains(n, s)) <= 1e-10
    ratio = ex.equalisation_ratio(g)
    print("ratio", ratio, "gains", g)
    assert ratio <= 0.5
    # and the final colours: the luma spread over the seen points shrinks
    seen = ref["top_frame"][:, 0] >= 0
    before, _ = ex.finalise(ref["top_score"], ref["top_rgb"], ref["top_frame"], np.ones(6))
    after, _ = ex.finalise(ref["top_score"], ref["top_rgb"], ref["top_frame"], g)
    assert np.std(after[seen, 0].astype(np.float64)) < 0.5 * np.std(before[seen, 0].astype(np.float64))


def test_exposure_entry_points_are_declared_and_exported():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for sym in ("pcp_view_pair_stats", "pcp_view_pair_stats_counters", "pcp_exposure_gains", "pcp_set_frame_gains"):
        assert sym in names and hasattr(lib, sym), sym
    assert lib.pcp_abi_version() == 6
    for m in ("view_pair_stats", "view_pair_stats_counters", "set_frame_gains"):
        assert callable(getattr(capi.Context, m))
    assert lib.pcp_view_pair_stats(None, None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_view_pair_stats_counters(None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_set_frame_gains(None, None, C.c_int32(0)) == capi.PCP_ERR_INVALID
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in ("pcp_view_pair_stats", "pcp_exposure_gains", "pcp_set_frame_gains"):
        assert sym in doc


def test_cli_balance_exposure_flag_is_checked_at_parse_time(tmp_path):
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    exe = host_build.build()["PointCloudProcessor"]
    base = ["-p", str(tmp_path / "none.pcd"), "-o", str(tmp_path / "odo.txt"), "-i", str(tmp_path) + "/"]
    for bad in ("2", "-1", "yes", ""):
        p = subprocess.run([exe] + base + ["--balanceExposure", bad], capture_output=True, text=True)
        assert p.returncode == 254 and "--balanceExposure" in p.stderr, (bad, p.stderr)
        assert "Couldn't read point cloud file." not in p.stderr
    for ok in ("0", "1"):
        p = subprocess.run([exe] + base + ["--balanceExposure", ok], capture_output=True, text=True)
        assert p.returncode == 254 and "Couldn't read point cloud file." in p.stderr, (ok, p.stderr)
    # the statistics' exchange over GPUs and streamed chunks is not built: refused up front
    for extra in (["--gpus", "2"], ["--streamColour", "1", "--enableMLS", "1"]):
        p = subprocess.run([exe] + base + ["--balanceExposure", "1"] + extra, capture_output=True, text=True)
        assert p.returncode == 254 and "--balanceExposure" in p.stderr, (extra, p.stderr)
        assert "Couldn't read point cloud file." not in p.stderr
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--balanceExposure" in p.stdout + p.stderr


def test_kernel_resources_of_the_exposure_kernels():
    import re

    from pointcloudprocessor_amd import _build

    _build.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_notes

    ks = kernel_notes.notes()
    names = kernel_notes.demangle([k.get("name", "?") for k in ks])
    table = {re.sub(r"\(.*", "", re.sub(r"^void ", "", nm)).replace("pcp::", ""): k for k, nm in zip(ks, names)}
    for name in ("k_pair_stats", "k_finalise_gained<false>", "k_finalise_gained<true>"):
        k = table[name]
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    # the plain finalise keeps its registers (the gained form is a kernel of its own)
    k = table["k_finalise"]
    assert (k["sgpr_count"], k["vgpr_count"], k.get("group_segment_fixed_size", 0), k.get("private_segment_fixed_size", 0)) == (16, 26, 0, 0)
