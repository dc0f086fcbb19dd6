"""CPU suite of the tile bounds with half-extents: host/tile_bounds_selftest.cpp runs the inflation the box form of the tile
classifier gives a tile's camera coordinates (csrc/pcp_tile_box.hpp, compiled for the host) against brute force -- corners and
interior points of random boxes transformed in fp32 under rigid and under wild matrices -- in the project's plain build and in
one with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded); the two read-only entry points the GPU suite
reads the order and the bounds through are declared, exported, bound and documented."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_output(p):
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"tile bounds: (\d+) tiles, (\d+) transformed points, 0 outside", p.stdout)
    assert m and int(m.group(1)) >= 5000 and int(m.group(2)) > 500000, p.stdout
    m = re.search(r"rigid matrices on flat boxes: (\d+) of (\d+)", p.stdout)
    assert m and int(m.group(2)) > 1000 and 2 * int(m.group(1)) > int(m.group(2)), p.stdout
    assert "tile_bounds_selftest: 0 outside" in p.stdout


def test_tile_bounds_selftest_passes_in_a_plain_build():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["tile_bounds_selftest"]
    _check_output(subprocess.run([exe, "5000"], capture_output=True, text=True))


def test_tile_bounds_selftest_passes_under_asan_and_ubsan(tmp_path):
    from pointcloudprocessor_amd import host_build

    exe = str(tmp_path / "tile_bounds_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", os.path.join(host_build.HOST, "tile_bounds_selftest.cpp"), "-o", exe], check=True, capture_output=True)
    _check_output(subprocess.run([exe, "5000"], capture_output=True, text=True))


def test_entry_points_are_declared_exported_bound_and_documented():
    from pointcloudprocessor_amd import _build, capi

    _build.build()
    lib = capi.load()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name, method in (("pcp_cloud_order", "cloud_order"), ("pcp_tile_bounds", "tile_bounds")):
        assert name in capi.declared_symbols() and hasattr(lib, name), name
        assert hasattr(capi.Context, method), method
        assert name in doc, name
    assert lib.pcp_abi_version() == 6
