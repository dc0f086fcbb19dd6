"""CPU suite of the visit's short forms (csrc/pcp_visit_forms.hpp): the header compiles for the host from the same text the
kernels use, and host/visit_forms_selftest.cpp checks the identities in plain C++ (std::fma, -ffp-contract=off) on random and
edge operands; the new self-test entry point is declared, exported, bound and documented, and the ABI version stays."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_visit_forms_selftest_passes_in_a_plain_build():
    from pointcloudprocessor_amd import host_build

    exe = host_build.build()["visit_forms_selftest"]
    p = subprocess.run([exe, "300000"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    for part in ("distortion", "cell", "sqrt"):
        m = re.search(part + r": (\d+) \w+, 0 mismatches", p.stdout)
        assert m and int(m.group(1)) > 100000, p.stdout
    assert "visit_forms_selftest: 0 mismatches" in p.stdout


def test_host_program_is_built_without_contraction():
    """the identities are statements about individually rounded operations: the recipe must say so"""
    with open(os.path.join(ROOT, "pointcloudprocessor_amd", "host_build.py")) as f:
        assert "-ffp-contract=off" in f.read()
    from pointcloudprocessor_amd import _build

    assert "-ffp-contract=off" in _build.HIPCC_FLAGS and "pcp_visit_forms.hpp" in _build.HEADERS


def test_entry_point_is_declared_exported_bound_and_documented(tmp_path):
    from pointcloudprocessor_amd import _build, capi

    _build.build()
    lib = capi.load()
    assert "pcp_selftest_visit_forms" in capi.declared_symbols() and hasattr(lib, "pcp_selftest_visit_forms")
    assert "pcp_selftest_arithmetic" in capi.declared_symbols() and hasattr(capi.Context, "selftest_visit_forms")
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "pcp_selftest_visit_forms" in f.read()
    src = tmp_path / "abi.c"
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n  (void)pcp_selftest_visit_forms;\n  (void)pcp_selftest_arithmetic;\n'
                   "  return PCP_ABI_VERSION == 6 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)
