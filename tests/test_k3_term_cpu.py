"""CPU suite of the short distortion without the k3 term (csrc/pcp_visit_forms.hpp, distort_short<false>): host/k3_term_selftest.cpp
runs it against the written form in plain C++ (std::fma, -ffp-contract=off) under cameras that qualify, on random operands and on a
sweep through the magnitudes where r6 overflows, and checks the host's condition (k3_term_droppable) on cameras that pass and that
fail -- in the project's plain build and in one with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded).  The
code objects of the two kernels that run the form keep their register bounds; the pinned k_colour_pass forms are left to
tests/test_label_fusion_cpu.py."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_output(p):
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"k3 term: (\d+) pairs \((\d+) with an overflowing r6\), 0 mismatches", p.stdout)
    assert m and int(m.group(1)) > 1000000 and int(m.group(2)) > 100000, p.stdout
    m = re.search(r"predicate: (\d+) cameras that keep the term, 0 mismatches", p.stdout)
    assert m and int(m.group(1)) >= 60, p.stdout
    assert "k3_term_selftest: 0 mismatches" in p.stdout


def test_k3_term_selftest_passes_in_a_plain_build():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["k3_term_selftest"]
    _check_output(subprocess.run([exe, "100000"], capture_output=True, text=True))


def test_k3_term_selftest_passes_under_asan_and_ubsan(tmp_path):
    from pointcloudprocessor_amd import host_build

    exe = str(tmp_path / "k3_term_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", os.path.join(host_build.HOST, "k3_term_selftest.cpp"), "-o", exe], check=True, capture_output=True)
    _check_output(subprocess.run([exe, "100000"], capture_output=True, text=True))


def _kernel_table():
    from pointcloudprocessor_amd import _build

    _build.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_notes

    ks = kernel_notes.notes()
    names = kernel_notes.demangle([k.get("name", "?") for k in ks])
    return {re.sub(r"\(.*", "", re.sub(r"^void ", "", nm)).replace("pcp::", ""): k for k, nm in zip(ks, names)}


def test_the_two_kernels_keep_their_register_bounds():
    """k_depth_pass<true, ...>: 8 waves (at most 64 VGPRs), nothing spilled; k_colour_pass_preload<...>: at most 61 VGPRs, no scratch
    -- with the term (the form a camera that does not qualify keeps) and without it."""
    table = _kernel_table()
    for name in ("k_depth_pass<true, true>", "k_depth_pass<true, false>"):
        k = table[name]
        print(name, k)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 64, (name, k)
        assert k.get("sgpr_spill_count", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, (name, k)
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
    for name in ("k_colour_pass_preload<true>", "k_colour_pass_preload<false>"):
        k = table[name]
        print(name, k)
        assert k["vgpr_count"] <= 61 and k.get("agpr_count", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, (name, k)
    # the form without the term is no larger than the one with it
    assert table["k_depth_pass<true, false>"]["vgpr_count"] <= table["k_depth_pass<true, true>"]["vgpr_count"]
    assert table["k_colour_pass_preload<false>"]["vgpr_count"] <= table["k_colour_pass_preload<true>"]["vgpr_count"]
    # the tile level without the `inside` words exists beside the one with them
    assert "k_tile_mask_dense<false>" in table and "k_tile_mask_dense<true>" in table


def test_entry_point_is_declared_exported_bound_and_documented():
    from pointcloudprocessor_amd import _build, capi

    _build.build()
    lib = capi.load()
    assert "pcp_selftest_k3_term" in capi.declared_symbols() and hasattr(lib, "pcp_selftest_k3_term")
    assert hasattr(capi.Context, "selftest_k3_term")
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "pcp_selftest_k3_term" in f.read()
    assert lib.pcp_abi_version() == 6
