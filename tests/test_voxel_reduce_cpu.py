"""CPU suite of the voxel-grid output (csrc/pcp_voxel_reduce.hpp through pcp_voxel_reduce_host: no context, no GPU) against the
restatement in _voxel_reduce_ref.py.  Every comparison is exact equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _voxel_reduce_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_voxel_reduce_begin", "pcp_voxel_reduce_add", "pcp_voxel_reduce_finish", "pcp_voxel_reduce_fetch", "pcp_voxel_reduce_stats",
       "pcp_voxel_reduce_end", "pcp_voxel_reduce_host")
LEAVES = (0.001, 0.013, 0.25, 1.0)


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


def _cloud(n=5000, seed=7):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-8.0, 8.0, (n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    label = rng.integers(0, 256, n, dtype=np.uint8)
    return xyz, rgb, label


def _equal(got, want, with_label=True):
    bad = ref.same(got, want, with_label)
    assert bad is None, f"{bad} differs"
    assert got["voxels"] == len(want["count"])


@pytest.mark.parametrize("leaf", LEAVES)
def test_host_form_equals_the_restatement(leaf):
    xyz, rgb, label = _cloud()
    got = _capi().voxel_reduce_host(leaf, xyz, rgb, label)
    want = ref.reduce(leaf, xyz, rgb, label)
    _equal(got, want)
    assert int(got["count"].sum()) == len(xyz)


@pytest.mark.parametrize("leaf", LEAVES)
def test_boundary_rows(leaf):
    lf = np.float32(leaf)
    vals = [np.float32(-0.0), np.float32(0.0), np.float32(1e-45), np.float32(-1e-45), np.float32(2.0 ** -9), np.float32(-(2.0 ** -9))]
    for k in range(-3, 4):
        v = np.float32(k) * lf
        vals += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
    vals = np.array(vals, np.float32)
    # every value on every axis, the other two axes held at a second value of the list
    rows = []
    for i, v in enumerate(vals):
        w = vals[(i + 5) % len(vals)]
        rows += [(v, w, w), (w, v, w), (w, w, v), (v, v, v)]
    xyz = np.array(rows, np.float32)
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (len(xyz), 3), dtype=np.uint8)
    label = rng.integers(0, 256, len(xyz), dtype=np.uint8)
    _equal(_capi().voxel_reduce_host(leaf, xyz, rgb, label), ref.reduce(leaf, xyz, rgb, label))


def test_single_row_voxels_return_their_rows():
    # a 5 mm lattice, jittered by less than 1 mm, |coordinate| >= 2^-9: no two points share a 1 mm voxel
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(*(np.arange(1, 13),) * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    sign = rng.choice([-1.0, 1.0], g.shape)
    xyz = (sign * (g * 0.005 + rng.uniform(0.0, 0.0009, g.shape))).astype(np.float32)
    assert np.abs(xyz).min() >= 2.0 ** -9
    rgb = rng.integers(0, 256, (len(xyz), 3), dtype=np.uint8)
    label = rng.integers(0, 256, len(xyz), dtype=np.uint8)
    got = _capi().voxel_reduce_host(0.001, xyz, rgb, label)
    keys = np.array([ref.key_of(c) for c in ref.cells(0.001, xyz)], dtype=object)
    assert len(set(keys.tolist())) == len(xyz)
    order = np.array(sorted(range(len(xyz)), key=lambda i: keys[i]))
    assert got["voxels"] == len(xyz) and (got["count"] == 1).all()
    assert got["xyz"].tobytes() == xyz[order].tobytes()
    assert got["rgb"].tobytes() == rgb[order].tobytes() and got["label"].tobytes() == label[order].tobytes()


def test_all_rows_in_one_voxel():
    rng = np.random.default_rng(5)
    n = 20000
    base = np.array([0.3125, -0.4375, 0.5625], np.float32)
    xyz = np.tile(base, (n, 1))
    xyz[n // 2:] += rng.uniform(-1e-3, 1e-3, (n - n // 2, 3)).astype(np.float32)  # half duplicated, half near-duplicated
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    label = rng.integers(0, 256, n, dtype=np.uint8)
    got = _capi().voxel_reduce_host(0.25, xyz, rgb, label)
    assert got["voxels"] == 1 and int(got["count"][0]) == n
    assert (got["rgb"][0] == rgb.astype(np.int64).sum(0) // n).all() and int(got["label"][0]) == int(label.astype(np.int64).sum()) // n
    fix = [sum(ref.fixed(v) for v in xyz[:, a]) for a in range(3)]
    want = np.array([np.float32(float((2 * f + n) // (2 * n)) * 2.0 ** -32) for f in fix], np.float32)
    assert got["xyz"][0].tobytes() == want.tobytes()
    _equal(got, ref.reduce(0.25, xyz, rgb, label))


@pytest.mark.parametrize("leaf", (0.013, 0.25))
def test_invariance_under_order_and_slicing(leaf):
    capi = _capi()
    xyz, rgb, label = _cloud(seed=19)
    got = capi.voxel_reduce_host(leaf, xyz, rgb, label)
    p = np.random.default_rng(23).permutation(len(xyz))
    again = capi.voxel_reduce_host(leaf, xyz[p], rgb[p], label[p])
    assert ref.same(again, got, True) is None
    sums = None
    for sl in (slice(0, 1700), slice(1700, 1701), slice(1701, None)):  # per-slice sums merged by the restatement
        sums = ref.accumulate(leaf, xyz[sl], rgb[sl], label[sl], sums)
    assert ref.same(got, ref.finish(leaf, sums), True) is None


def test_refusals_and_capacity():
    capi = _capi()
    xyz, rgb, label = _cloud(64)
    for leaf in (float("nan"), 0.0, 9e-5, 1.5, -0.01, float("inf")):
        with pytest.raises(capi.PcpError) as e:
            capi.voxel_reduce_host(leaf, xyz, rgb, label)
        assert e.value.code == capi.PCP_ERR_INVALID, leaf
    far = xyz.copy()
    far[10, 1] = 200.0
    with pytest.raises(capi.PcpError) as e:
        capi.voxel_reduce_host(1e-4, far, rgb, label)
    assert e.value.code == capi.PCP_ERR_RANGE
    assert capi.voxel_reduce_host(1e-4, xyz, rgb, label)["voxels"] == 64  # (8 m at 1e-4 is inside the range)
    for v in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[3, 2] = v
        with pytest.raises(capi.PcpError) as e:
            capi.voxel_reduce_host(0.25, bad, rgb, label)
        assert e.value.code == capi.PCP_ERR_RANGE
    full = capi.voxel_reduce_host(1.0, xyz, rgb, label)
    part = capi.voxel_reduce_host(1.0, xyz, rgb, label, capacity=5)
    assert part["voxels"] == full["voxels"] > 5 and part["xyz"].tobytes() == full["xyz"][:5].tobytes()
    none = capi.voxel_reduce_host(1.0, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    assert none["voxels"] == 0 and "label" not in none
    lib = capi.load()
    for f in ("begin", "add", "finish", "stats", "end"):  # no context: an argument error, not a crash
        fn = getattr(lib, "pcp_voxel_reduce_" + f)
        args = {"begin": (None, C.c_float(0.01), C.c_int64(0)), "end": (None,)}.get(f, (None, None))
        assert fn(*args) == capi.PCP_ERR_INVALID, f


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    for m in ("voxel_reduce_begin", "voxel_reduce_add", "voxel_reduce_finish", "voxel_reduce_fetch", "voxel_reduce_stats", "voxel_reduce_end"):
        assert callable(getattr(capi.Context, m)), m
    assert callable(capi.voxel_reduce_host) and lib.pcp_abi_version() == 6 and capi.K_COUNT == 13


def test_header_with_the_new_declarations_is_plain_c(tmp_path):
    src = tmp_path / "abi.c"
    calls = "\n".join(f"  (void){s};" for s in NEW)
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n' + calls + "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["voxel_reduce_selftest"]
    out = subprocess.run([exe, "200000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
