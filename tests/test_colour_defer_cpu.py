"""CPU suite of the deferred texel fetch of the whole-run colour call (k_colour_pass_deferred, csrc/pcp_colour.hip): the host's
condition for it (deferred_index_fits, csrc/pcp_colour_defer.hpp) at its edges -- a range of exactly 2^32 texels, one keyframe
more, the pixel counts of both cameras -- through host/colour_defer_selftest.cpp in the project's plain build and in one with
AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded); the registers of the new kernel against those of the
kernel it stands in for, from the code object's metadata; and the switch's place in the documents."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HD, REF = 1920 * 1080, 4096 * 3000  # the bench's camera and the reference's
# (begin, end, image_px) -> fits.  2^32 = 2071.2 x HD = 349.5 x REF = 65536 x 65536.
EDGES = [
    ((0, 65536, 65536), 1),      # exactly 2^32 texels: the last index is 2^32 - 1
    ((0, 65537, 65536), 0),      # one keyframe more
    ((0, 65536, 65537), 0),      # one pixel more per image
    ((9, 65545, 65536), 1),      # the range's length counts, not its end
    ((9, 65546, 65536), 0),
    ((0, 2071, HD), 1),
    ((0, 2072, HD), 0),
    ((100, 2171, HD), 1),
    ((100, 2172, HD), 0),
    ((0, 256, HD), 1),           # the bench
    ((0, 349, REF), 1),
    ((0, 350, REF), 0),
    ((31, 380, REF), 1),
    ((31, 381, REF), 0),
    ((0, 256, REF), 1),          # the bench's camera_ref step
    ((4, 4, HD), 0),             # no range
    ((0, 1, 0), 0),              # no image
]


def _check(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"colour_defer_selftest: (\d+) cases, 0 mismatches", p.stdout)
    assert m and int(m.group(1)) >= 150, p.stdout
    args = [str(v) for (triple, _) in EDGES for v in triple]
    p = subprocess.run([exe] + args, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == len(EDGES), p.stdout
    for line, ((b, e, px), want) in zip(lines, EDGES):
        assert line == f"fits {b} {e} {px}: {want}", (line, want)


def test_condition_at_its_edges_in_a_plain_build():
    from pointcloudprocessor_amd import host_build

    _check(host_build.build()["colour_defer_selftest"])


def test_condition_at_its_edges_under_asan_and_ubsan(tmp_path):
    from pointcloudprocessor_amd import host_build

    exe = str(tmp_path / "colour_defer_selftest_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    os.path.join(host_build.HOST, "colour_defer_selftest.cpp"), "-o", exe], check=True, capture_output=True)
    _check(exe)


def _kernel_table():
    from pointcloudprocessor_amd import _build

    _build.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_notes

    ks = kernel_notes.notes()
    names = kernel_notes.demangle([k.get("name", "?") for k in ks])
    return {re.sub(r"\(.*", "", re.sub(r"^void ", "", nm)).replace("pcp::", ""): k for k, nm in zip(ks, names)}


def test_the_deferred_kernel_needs_no_more_registers_than_the_one_it_stands_in_for():
    """No scratch, nothing spilled to memory, and at most the VGPRs of k_colour_pass_preload -- 61 with the k3 term, 60 without it,
    the figures of the commit before the deferred kernel -- so the waves per SIMD are at least that kernel's."""
    table = _kernel_table()
    for k3, parent_vgprs in (("true", 61), ("false", 60)):
        new, old = table[f"k_colour_pass_deferred<{k3}>"], table[f"k_colour_pass_preload<{k3}>"]
        print(k3, new, old)
        assert new["vgpr_count"] <= parent_vgprs and new["vgpr_count"] <= old["vgpr_count"], (new, old)
        assert new.get("agpr_count", 0) == 0 and new.get("vgpr_spill_count", 0) == 0, new
        assert new.get("private_segment_fixed_size", 0) == 0 and new.get("group_segment_fixed_size", 0) == 0, new
    assert table["k_colour_pass_deferred<false>"]["vgpr_count"] <= table["k_colour_pass_deferred<true>"]["vgpr_count"]


def test_the_switch_is_documented_and_in_the_switch_matrix():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "PCP_COLOUR_DEFER" in f.read()
    with open(os.path.join(ROOT, "scripts", "switch_matrix.sh")) as f:
        assert "PCP_COLOUR_DEFER=0" in f.read()
