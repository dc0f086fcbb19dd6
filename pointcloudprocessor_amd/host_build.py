"""g++ build of the C++ host side above the C ABI (pointcloudprocessor_amd/host/)."""
from __future__ import annotations

import glob
import os
import subprocess

from . import _build

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
BIN = os.path.join(HOST, "bin")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

TARGETS = {
    "pcp_shim_selftest": ["shim_selftest.cpp"],
    "PointCloudProcessor": ["main.cpp"],
    "image_dump": ["image_dump.cpp"],
    "format_selftest": ["format_selftest.cpp"],
    "parse_selftest": ["parse_selftest.cpp"],  # csrc/pcp_ascii_parse.hpp compiled for the host (CPU only: never a GPU job)
    "visit_forms_selftest": ["visit_forms_selftest.cpp"],  # csrc/pcp_visit_forms.hpp compiled for the host (CPU only)
    "k3_term_selftest": ["k3_term_selftest.cpp"],  # csrc/pcp_visit_forms.hpp, the form without the k3 term (CPU only)
    "voxel_reduce_selftest": ["voxel_reduce_selftest.cpp"],  # csrc/pcp_voxel_reduce.hpp compiled for the host (CPU only)
    "normals_selftest": ["normals_selftest.cpp"],  # csrc/pcp_normals.hpp compiled for the host (CPU only)
    "compare_selftest": ["compare_selftest.cpp"],  # csrc/pcp_compare.hpp compiled for the host (CPU only)
    "register_selftest": ["register_selftest.cpp"],  # csrc/pcp_register.hpp compiled for the host (CPU only)
    "coarse_selftest": ["coarse_selftest.cpp"],  # csrc/pcp_coarse.hpp compiled for the host (CPU only)
    "ortho_selftest": ["ortho_selftest.cpp"],  # csrc/pcp_ortho.hpp compiled for the host (CPU only)
    "ortho_texture_selftest": ["ortho_texture_selftest.cpp"],  # csrc/pcp_ortho_texture.hpp compiled for the host (CPU only)
    "crack_width_selftest": ["crack_width_selftest.cpp"],  # csrc/pcp_crack_width.hpp compiled for the host (CPU only)
    "crack_fuse_selftest": ["crack_fuse_selftest.cpp"],  # csrc/pcp_crack_fuse.hpp compiled for the host (CPU only)
    "crack_length_selftest": ["crack_length_selftest.cpp"],  # csrc/pcp_crack_length.hpp compiled for the host (CPU only)
    "crack_skeleton_selftest": ["crack_skeleton_selftest.cpp"],  # csrc/pcp_crack_skeleton.hpp compiled for the host (CPU only)
    "crack_direction_selftest": ["crack_direction_selftest.cpp"],  # csrc/pcp_crack_direction.hpp compiled for the host (CPU only)
    "crack_branch_selftest": ["crack_branch_selftest.cpp"],  # csrc/pcp_crack_branch.hpp compiled for the host (CPU only)
    "image_balance_selftest": ["image_balance_selftest.cpp"],  # csrc/pcp_image_balance.hpp compiled for the host (CPU only)
    "ortho_cyl_selftest": ["ortho_cyl_selftest.cpp"],  # csrc/pcp_ortho_cyl.hpp compiled for the host (CPU only)
    "ortho_cyl_texture_selftest": ["ortho_cyl_texture_selftest.cpp"],  # csrc/pcp_ortho_cyl.hpp's way back, pixel to point (CPU only)
    "ortho_defects_selftest": ["ortho_defects_selftest.cpp"],  # csrc/pcp_ortho_defects.hpp compiled for the host (CPU only)
    "facets_selftest": ["facets_selftest.cpp"],  # csrc/pcp_facets.hpp compiled for the host (CPU only)
    "tile_bounds_selftest": ["tile_bounds_selftest.cpp"],  # csrc/pcp_tile_box.hpp compiled for the host (CPU only)
    "colour_defer_selftest": ["colour_defer_selftest.cpp"],  # csrc/pcp_colour_defer.hpp compiled for the host (CPU only)
    "options_probe": ["options_probe.cpp"],  # host/cli_options.hpp: parses command lines from stdin (CPU only: never a GPU job)
}


def header_deps() -> list:
    """The headers every target is taken to depend on: all of host/ and csrc/, and the C ABI."""
    return sorted(glob.glob(os.path.join(HOST, "*.hpp"))) + sorted(glob.glob(os.path.join(_build.CSRC, "*.hpp"))) + [
        os.path.join(_build.INCLUDE, "pcp_hip.h")]


def build(force: bool = False) -> dict:
    os.makedirs(BIN, exist_ok=True)
    out = {}
    for name, srcs in TARGETS.items():
        exe = os.path.join(BIN, name)
        deps = [os.path.join(HOST, s) for s in srcs] + header_deps()
        stale = force or not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps)
        if stale:
            extra = os.environ.get("PCP_HOST_CXXFLAGS", "").split()  # e.g. -fsanitize=address,undefined (CPU-side checks)
            # the multi-GPU host (pcp_multi.hpp) calls the HIP runtime and RCCL directly: host-only API use, plain g++
            multi = ["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include")] if name == "PointCloudProcessor" else []
            multi_libs = ["-L", os.path.join(ROCM, "lib"), "-lrccl", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")] \
                if name == "PointCloudProcessor" else []
            # (-ffp-contract=off: the visit forms are checked operation by operation, as the device library is built)
            cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra"] + extra + multi + ["-I", _build.INCLUDE, "-I", HOST] + [
                os.path.join(HOST, s) for s in srcs] + ["-L", _build.LIB_DIR, "-lpcp_hip"] + multi_libs + [
                                                        "-lz", "-Wl,-rpath,$ORIGIN/../../lib", "-o", exe]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            if proc.returncode != 0:
                raise RuntimeError(f"g++ failed for {name}:\n{proc.stderr[-3000:]}")
        out[name] = exe
    return out
