"""Fused segmentation labels, the part that needs no GPU: the restatement the GPU tests expect against (exact integers
vs. fractions.Fraction), its known answers, the new ABI surface, the CLI's flag checks and the cross-compiled kernels'
resource notes."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _label_fusion_ref as lf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scores(rng, k):
    """fp32 scores as final_score makes them: in [0.2, 1], with full mantissas"""
    s = rng.uniform(0.2, 1.0, k).astype(np.float32)
    s[rng.random(k) < 0.1] = np.float32(1.0)
    s[rng.random(k) < 0.1] = np.float32(0.2)
    return s


def test_integer_fusion_is_the_floor_of_the_rational_mean():
    rng = np.random.default_rng(5)
    for _ in range(4000):
        k = int(rng.integers(1, 6))
        s = _scores(rng, k)
        m = rng.integers(0, 256, k)
        if rng.random() < 0.3:
            m[rng.random(k) < 0.6] = 255
        label, hits, views = lf.fuse(s, m)
        assert label == lf.fuse_fraction(s, m)
        assert hits == int((m == 255).sum()) and views == k
        assert min(m) <= label <= max(m)


def test_array_form_equals_the_scalar_form():
    rng = np.random.default_rng(6)
    n = 3000
    ts = np.full((n, 5), -1.0, np.float32)
    tf = np.full((n, 5), -1, np.int32)
    tm = np.zeros((n, 5), np.uint8)
    for i in range(n):
        k = int(rng.integers(0, 6))
        ts[i, :k] = np.sort(_scores(rng, k))[::-1]
        tf[i, :k] = rng.integers(0, 24, k)
        tm[i, :k] = rng.integers(0, 256, k) if rng.random() < 0.7 else 255
    label, hits, views = lf.fuse_arrays(ts, tf, tm)
    for i in range(n):
        k = int((tf[i] >= 0).sum())
        assert (int(label[i]), int(hits[i]), int(views[i])) == lf.fuse(ts[i, :k], tm[i, :k]), i
    assert (views == 0).any() and not label[views == 0].any() and not hits[views == 0].any()


def test_known_answers():
    # every fp32 score in [2^-3, 2) is an integer number of 2^-26
    for s in (0.125, 0.2, np.nextafter(np.float32(0.2), np.float32(1)), 0.25, 0.5, 1.0, np.nextafter(np.float32(2), np.float32(0))):
        assert 0 < lf.score_units(np.float32(s)) < 1 << 27
    with pytest.raises(ValueError):
        lf.score_units(np.nextafter(np.float32(0.125), np.float32(0)))  # below 2^-3 the ulp is 2^-27
    # a single view returns its mask value, whatever its score
    sweep = np.concatenate([np.linspace(0.2, 1.0, 97).astype(np.float32), _scores(np.random.default_rng(7), 64)])
    for m in range(256):
        for s in sweep:
            assert lf.fuse([s], [m]) == (m, int(m == 255), 1)
    # all views 255 -> 255 (an fp32 mean truncates many of these to 254)
    rng = np.random.default_rng(8)
    truncated = 0
    for _ in range(2000):
        k = int(rng.integers(1, 6))
        s = _scores(rng, k)
        assert lf.fuse(s, [255] * k) == (255, k, k)
        tot = np.float32(0)
        acc = np.float32(0)
        for v in s:
            acc = np.float32(acc + np.float32(255) * v)
            tot = np.float32(tot + v)
        truncated += int(np.float32(acc / tot)) < 255
    assert truncated > 0
    # entries of equal score in any order
    for _ in range(200):
        s = np.float32(rng.uniform(0.2, 1.0))
        k = int(rng.integers(2, 6))
        m = list(rng.integers(0, 256, k))
        want = lf.fuse([s] * k, m)
        for perm in itertools.islice(itertools.permutations(range(k)), 24):
            assert lf.fuse([s] * k, [m[j] for j in perm]) == want
    # the empty list
    assert lf.fuse([], []) == (0, 0, 0)


def test_label_entry_points_are_declared_and_exported():
    from pointcloudprocessor_amd import _build, capi

    _build.build()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in ("pcp_set_label_fusion", "pcp_colour_labels", "pcp_colour_labels_device"):
        assert s in names and hasattr(lib, s), s
    assert lib.pcp_abi_version() == 6
    assert capi.K_COUNT == 13
    for m in ("set_label_fusion", "colour_labels", "colour_labels_device"):
        assert callable(getattr(capi.Context, m))
    # no context: an argument error, not a crash
    assert lib.pcp_set_label_fusion(None, C.c_int32(1)) == capi.PCP_ERR_INVALID
    assert lib.pcp_colour_labels(None, None, None, None) == capi.PCP_ERR_INVALID
    assert lib.pcp_colour_labels_device(None, None, None) == capi.PCP_ERR_INVALID
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in ("pcp_set_label_fusion", "pcp_colour_labels", "pcp_colour_labels_device"):
        assert s in doc


def test_cli_fuse_masks_flag_is_checked_at_parse_time(tmp_path):
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    exe = host_build.build()["PointCloudProcessor"]
    base = ["-p", str(tmp_path / "none.pcd"), "-o", str(tmp_path / "odo.txt"), "-i", str(tmp_path) + "/"]
    # without -m: a parse-time error (exit -2), before the point cloud is even looked for
    p = subprocess.run([exe] + base + ["--fuseMasks", "1"], capture_output=True, text=True)
    assert p.returncode == 254 and "--fuseMasks" in p.stderr and "mask_image_folder" in p.stderr
    assert "Couldn't read point cloud file." not in p.stderr
    for bad in ("2", "-1", "yes", "1.5", ""):
        p = subprocess.run([exe] + base + ["-m", str(tmp_path) + "/", "--fuseMasks", bad], capture_output=True, text=True)
        assert p.returncode == 254 and "--fuseMasks" in p.stderr, (bad, p.stderr)
        assert "Couldn't read point cloud file." not in p.stderr
    # accepted values reach the loader (and fail there: no such file)
    for ok in ("0", "1"):
        p = subprocess.run([exe] + base + ["-m", str(tmp_path) + "/", "--fuseMasks", ok], capture_output=True, text=True)
        assert p.returncode == 254 and "Couldn't read point cloud file." in p.stderr, (ok, p.stderr)
    # 0 without -m is the reference's behaviour: allowed
    p = subprocess.run([exe] + base + ["--fuseMasks", "0"], capture_output=True, text=True)
    assert p.returncode == 254 and "Couldn't read point cloud file." in p.stderr


# registers / LDS / scratch of the colour-stage kernels as they were before the label form existed (gfx950, the build's
# flags): sgpr, vgpr, lds, scratch.  The fusion-off path launches exactly these.
BEFORE = {
    "k_finalise": (16, 26, 0, 0),
    "k_match_fixup<false>": (106, 59, 0, 0),
    "k_colour_pass<false, 0, false, false>": (106, 55, 0, 0),
    "k_colour_pass<false, 3, false, false>": (106, 59, 0, 0),
    "k_colour_pass<true, 1, false, false>": (106, 56, 0, 0),
    "k_colour_pass<true, 1, true, false>": (106, 55, 0, 0),
    "k_colour_pass<true, 2, false, false>": (105, 61, 0, 0),
    "k_colour_pass<true, 2, true, false>": (106, 61, 0, 0),
    "k_colour_pass<true, 3, false, false>": (106, 63, 0, 0),
    "k_colour_pass<true, 3, true, false>": (106, 61, 0, 0),
}
LABEL_FORMS = ["k_finalise_labels", "k_match_fixup<true>"] + [
    k.replace(", false>", ", true>") for k in BEFORE if k.startswith("k_colour_pass")]


def test_kernel_resources_label_forms_have_no_scratch_and_the_old_forms_are_untouched():
    import re

    from pointcloudprocessor_amd import _build

    _build.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_notes

    ks = kernel_notes.notes()
    names = kernel_notes.demangle([k.get("name", "?") for k in ks])
    table = {}
    for k, nm in zip(ks, names):
        short = re.sub(r"\(.*", "", re.sub(r"^void ", "", nm)).replace("pcp::", "")
        table[short] = k
    for name, (sgpr, vgpr, lds, scratch) in BEFORE.items():
        k = table[name]
        got = (k["sgpr_count"], k["vgpr_count"], k.get("group_segment_fixed_size", 0), k.get("private_segment_fixed_size", 0))
        assert got == (sgpr, vgpr, lds, scratch), (name, got)
        assert k.get("vgpr_spill_count", 0) == 0
    assert len(LABEL_FORMS) == 10
    for name in LABEL_FORMS:
        k = table[name]
        assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, (name, k)
        assert k.get("group_segment_fixed_size", 0) == 0, name
    # the label form of a colour pass costs no vector register over its colour-only twin
    for name in BEFORE:
        if name.startswith("k_colour_pass"):
            assert table[name.replace(", false>", ", true>")]["vgpr_count"] <= table[name]["vgpr_count"], name
