"""CPU suite of the crack widths on the map (csrc/pcp_crack_fuse.hpp through pcp_crack_fuse_host and
pcp_crack_components_host: no context, no GPU) against the restatement in _crack_fuse_ref.py, by exact equality."""
import os
import subprocess

import numpy as np
import pytest

import _crack_fuse_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcp_crack_fuse_begin", "pcp_crack_fuse_add", "pcp_crack_fuse_fetch", "pcp_crack_fuse_end", "pcp_crack_fuse_host",
       "pcp_crack_components", "pcp_crack_components_fetch", "pcp_crack_components_host")
RADIUS = 0.005
HALF_QUANTUM = np.float32(2.5 / 1048576.0)  # a tie: 2.5 quanta round to 2
SPECIAL_WIDTHS = np.array([0.0, HALF_QUANTUM, 1.5 / 1048576.0, 2047.9999, 2048.0, 1e6, 0.003], np.float32)


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


def _frames(shape, n, seed, frames=6):
    """per keyframe: (index, pixel, range, flags, width) -- synthetic contributor lists over an image of `shape`.  Point 0 is
    credited in every keyframe, point n - 1 (n > 1) is listed everywhere and credited nowhere; point 1 (n > 2) meets
    keyframes 4 and 2 at one range."""
    h, w = shape
    rng = np.random.default_rng(seed)
    out = []
    for f in range(frames):
        flags = rng.choice(np.array([0, 1, 1 | 2, 64 | 1, 64 | 2 | 1, 64 | 60 | 1], np.uint8), (h, w))
        width = rng.uniform(0.0, 0.01, (h, w)).astype(np.float32)
        special = rng.random((h, w)) < 0.2
        width[special] = rng.choice(SPECIAL_WIDTHS, int(special.sum()))
        index = np.sort(rng.choice(n, max(1, int(0.7 * n)), replace=False)).astype(np.int32) if n > 1 else np.zeros(1, np.int32)
        index = np.union1d(index, [0, n - 1] + ([1] if n > 2 else [])).astype(np.int32)
        pixel = rng.integers(0, h * w, len(index)).astype(np.int32)
        rg = rng.uniform(0.5, 9.0, len(index)).astype(np.float32)
        if h * w > 1:
            with_w = np.flatnonzero((flags.ravel() & 64) != 0)
            without = np.flatnonzero((flags.ravel() & 64) == 0)
            if len(with_w) == 0:
                flags.ravel()[0] |= 64
                with_w = np.array([0])
            if len(without) == 0:
                flags.ravel()[-1] = 1
                without = np.array([h * w - 1])
                with_w = with_w[with_w != h * w - 1]
            pixel[index == 0] = with_w[f % len(with_w)]
            if n > 1:
                pixel[index == n - 1] = without[f % len(without)]
            if n > 2:
                pixel[index == 1] = with_w[(3 * f + 1) % len(with_w)]
        else:
            flags[:] = 64 | 2 | 1 if f % 2 == 0 else 1  # one pixel: all or nobody is credited
        if n > 2 and f in (2, 4):
            rg[index == 1] = np.float32(0.25)  # the closest range of point 1, twice
        out.append((index, pixel, rg, flags, width))
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("shape", [(1, 1), (45, 70), (33, 129)], ids=lambda s: "%dx%d" % s)
def test_fuse_host_equals_the_restatement_in_two_orders(shape, n):
    capi = _capi()
    frames = _frames(shape, n, seed=1000 * shape[0] + n)
    want = ref.new_state(n)
    credited = [ref.add_frame(want, *fr[:3], f, *fr[3:]) for f, fr in enumerate(frames)]
    states = []
    for order in (range(6), (4, 1, 5, 0, 3, 2)):
        st = capi.crack_fuse_state(n)
        for f in order:
            index, pixel, rg, flags, width = frames[f]
            assert capi.crack_fuse_host(st, index, pixel, rg, f, flags, width) == credited[f]
        states.append(st)
    for k in ref.FIELDS:
        assert states[0][k].dtype == want[k].dtype
        assert np.array_equal(states[0][k], want[k]), k
        assert states[0][k].tobytes() == states[1][k].tobytes(), k
    st = states[0]
    assert (st["seen"] >= st["views"]).all() and (st["views"] >= st["centres"]).all()
    if shape != (1, 1):
        assert st["views"][0] == 6  # credited in every keyframe
        if n > 1:
            assert st["seen"][n - 1] == 6 and st["views"][n - 1] == 0 and st["min_q"][n - 1] == ref.NO_MIN and st["best_key"][n - 1] == ref.NO_KEY
        if n > 2:  # the equal-range tie goes to the lower keyframe
            assert st["views"][1] == 6 and int(st["best_key"][1] & np.uint64(0xFFFFFFFF)) == 2
            assert int(st["best_key"][1] >> np.uint64(32)) == int(np.float32(0.25).view(np.uint32))
    else:
        assert st["views"][0] == 3 and st["seen"][0] == 6
    res = ref.results(st)
    assert res["best_frame"][st["views"] == 0].tolist() == [-1] * int((st["views"] == 0).sum())
    assert (ref.fused_w(st)[st["views"] > 0] >= st["min_q"][st["views"] > 0]).all()
    assert (ref.fused_w(st)[st["views"] > 0] <= st["max_q"][st["views"] > 0]).all()


def test_quanta_of_the_special_widths():
    capi = _capi()
    flags = np.full((1, len(SPECIAL_WIDTHS)), 64, np.uint8)
    width = SPECIAL_WIDTHS[None, :].copy()
    n = len(SPECIAL_WIDTHS)
    st = capi.crack_fuse_state(n)
    capi.crack_fuse_host(st, np.arange(n), np.arange(n), np.ones(n), 0, flags, width)
    below = int(np.rint(float(np.float32(2047.9999)) * 2 ** 20))
    assert st["sum_q"].tolist() == [0, 2, 2, below, 2 ** 31 - 1, 2 ** 31 - 1, 3146]
    assert np.array_equal(st["sum_q"], ref.quantum(SPECIAL_WIDTHS))
    assert below < 2 ** 31 - 1


@pytest.fixture(scope="module")
def cases():
    out = ref.component_cases(RADIUS)
    for xyz, views, _ in out.values():
        xyz.setflags(write=False)
        views.setflags(write=False)
    return out


CASE_NAMES = ["chain_shuffled", "chain_descending", "chains_touch", "chains_apart", "duplicates", "ring", "one_cell", "non_finite",
              "min_views_1", "min_views_3", "single", "no_crack_point", "uniform"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_components_host_equals_the_restatement_and_scipy(cases, name):
    capi = _capi()
    assert set(CASE_NAMES) == set(cases)
    xyz, views, min_views = cases[name]
    label = capi.crack_components_host(xyz, views, min_views, RADIUS)
    want = ref.check_labels(label, xyz, views, min_views, RADIUS)
    sizes = np.bincount(want[want >= 0], minlength=1)
    comps = int((sizes > 0).sum())
    if name.startswith("chain_"):
        assert comps == 1 and (label == 0).all()
    elif name == "chains_touch":
        assert comps == 1
    elif name == "chains_apart":
        assert comps == 2 and sorted(np.unique(label).tolist()) == [0, 40]
    elif name == "ring":
        assert comps == 1
    elif name == "one_cell":
        assert comps == 1
    elif name == "non_finite":
        assert (label[~np.isfinite(xyz).all(axis=1)] == -1).all() and comps > 1
    elif name == "min_views_3":
        assert (label[views < 3] == -1).all() and (label[views >= 3] >= 0).all()
    elif name == "single":
        assert label.tolist() == [0]
    elif name == "no_crack_point":
        assert (label == -1).all() and comps == 0
    elif name == "uniform":
        assert comps > 10 and sizes.max() > 100, (comps, int(sizes.max()))
    elif name == "duplicates":
        assert np.array_equal(label[120:160], label[0:120:3]) and np.array_equal(label[160:], label[0:120:5])


def test_components_host_at_another_radius(cases):
    """the chain at the default radius breaks into singletons when it is spaced for a smaller one, and joins at a larger one"""
    capi = _capi()
    xyz, views, _ = cases["chain_shuffled"]
    few = xyz[np.argsort(xyz[:, 0])[:300]]
    assert len(np.unique(capi.crack_components_host(few, np.ones(300, np.uint32), 1, 0.02))) == 1
    wide = (few * np.float32(8.0)).astype(np.float32)  # spaced 0.036: beyond 0.02
    assert np.array_equal(capi.crack_components_host(wide, np.ones(300, np.uint32), 1, 0.02), np.arange(300))


def test_error_returns():
    capi = _capi()
    C = capi.C
    L = capi.load()
    xyz = np.zeros((4, 3), np.float32)
    views = np.ones(4, np.uint32)
    for mv, r in ((0, 0.02), (4097, 0.02), (1, 0.004), (1, 1.5), (1, float("nan"))):
        with pytest.raises(capi.PcpError) as e:
            capi.crack_components_host(xyz, views, mv, r)
        assert e.value.code == capi.PCP_ERR_INVALID, (mv, r)
    label = np.empty(4, np.int32)
    assert L.pcp_crack_components_host(C.c_int64(65537), capi._ptr(xyz), capi._ptr(views), C.c_int32(1), C.c_float(0.02), capi._ptr(label), None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_components_host(C.c_int64(4), None, capi._ptr(views), C.c_int32(1), C.c_float(0.02), capi._ptr(label), None) == capi.PCP_ERR_INVALID
    assert L.pcp_crack_components_host(C.c_int64(0), None, None, C.c_int32(1), C.c_float(0.02), None, None) == capi.PCP_OK
    # the fusion: a bad entry changes nothing
    st = capi.crack_fuse_state(3)
    flags = np.full((2, 2), 64, np.uint8)
    width = np.full((2, 2), 0.001, np.float32)
    for index, pixel, rg in (([0, 3], [0, 1], [1.0, 1.0]), ([0, -1], [0, 1], [1.0, 1.0]), ([0, 1], [0, 4], [1.0, 1.0]), ([0, 1], [0, -1], [1.0, 1.0]),
                             ([0, 1], [0, 1], [1.0, 0.0]), ([0, 1], [0, 1], [1.0, float("nan")]), ([0, 1], [0, 1], [-1.0, 1.0])):
        with pytest.raises(capi.PcpError) as e:
            capi.crack_fuse_host(st, index, pixel, rg, 0, flags, width)
        assert e.value.code == capi.PCP_ERR_INVALID
        fresh = capi.crack_fuse_state(3)
        assert all(np.array_equal(st[k], fresh[k]) for k in st)
    with pytest.raises(capi.PcpError) as e:
        capi.crack_fuse_host(st, [0], [0], [1.0], -1, flags, width)
    assert e.value.code == capi.PCP_ERR_INVALID
    assert capi.crack_fuse_host(st, [], [], [], 0, flags, width) == 0
    with pytest.raises(ValueError):
        capi.crack_fuse_host(dict(st, seen=st["seen"].astype(np.int64)), [0], [0], [1.0], 0, flags, width)


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    for m in ("crack_fuse_begin", "crack_fuse_add", "crack_fuse_fetch", "crack_fuse_end", "crack_components"):
        assert callable(getattr(capi.Context, m)), m
    assert callable(capi.crack_fuse_host) and callable(capi.crack_components_host)
    assert lib.pcp_abi_version() == 6 and capi.K_COUNT == 13
    assert capi.C.sizeof(capi.CrackLinkParams) == 8 and capi.C.sizeof(capi.CrackParams) == 8


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  pcp_crack_link_params p = {1, 0.02f};\n  (void)p;\n  ' +
                   "\n  ".join(f"(void){s};" for s in NEW) +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && sizeof(pcp_crack_link_params) == 8 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_selftest_builds_and_passes():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["crack_fuse_selftest"]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """The shared header's code in a stand-alone program of its own, address and undefined-behaviour sanitizers, on the CPU."""
    src = os.path.join(ROOT, "pointcloudprocessor_amd", "host", "crack_fuse_selftest.cpp")
    exe = str(tmp_path / "crack_fuse_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


def test_pipeline_refuses_index_shards():
    from pointcloudprocessor_amd import pipeline

    with pytest.raises(ValueError) as e:
        pipeline.PointCloudColorizer(None, rank=0, world=2).crack_map()
    assert "index shard" in str(e.value) and "not built" in str(e.value)
