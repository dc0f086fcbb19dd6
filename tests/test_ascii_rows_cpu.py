"""CPU suite of the device PCD writer's formatter (csrc/pcp_ascii.hpp through pcp_ascii_rows_host: no context, no GPU): the
bytes of '%.8g' on every exponent, both signs, the ties and carries of round-half-even, NaN / inf / zeros / subnormals; the
rgb and segmentMask columns; row bounds; the capacity contract; the header as plain C."""
import os
import subprocess

import numpy as np
import pytest

import _ascii_ref as ref

NEW = ("pcp_ascii_row_bound", "pcp_ascii_rows_host", "pcp_ascii_rows", "pcp_colour_compact_ascii", "pcp_mls_fetch_ascii")


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


def test_the_listed_ties_and_carries_print_as_glibc_prints_them():
    vals = np.array(list(ref.TIES), np.float32)
    assert [t.decode() for t in ref.g8(vals)] == list(ref.TIES.values())  # the Python expectation itself
    text = _capi().ascii_rows_host(ref.XYZI, ref.as_rows(vals, 4)).tobytes()
    assert text == ref.float_rows_text(ref.g8(vals), 4), ref.first_difference(text, ref.float_rows_text(ref.g8(vals), 4))


@pytest.mark.parametrize("kind", [ref.XYZI, ref.POINTNORMAL])
def test_every_exponent_both_signs(kind):
    capi = _capi()
    vals, texts = ref.value_set(), ref.value_text()
    assert len(vals) > 770000 and max(len(t) for t in texts) == 14
    nf = ref.FLOATS[kind]
    want = ref.float_rows_text(texts, nf)
    got = capi.ascii_rows_host(kind, ref.as_rows(vals, nf)).tobytes()
    assert got == want, ref.first_difference(got, want)
    assert max(len(r) for r in got.split(b"\n")) + 1 <= ref.BOUND[kind]


def test_rgb_and_mask_columns():
    capi = _capi()
    lv = np.array([0, 1, 255], np.uint8)
    rgb = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(-1, 3)  # {0, 1, 255}^3
    masks = np.array([0, 9, 10, 255, 65535], np.uint16)
    rgb = np.repeat(rgb, len(masks), 0)
    mask = np.tile(masks, 27)
    f = ref.as_rows(np.arange(3 * len(rgb), dtype=np.float32) * np.float32(-0.37), 3)
    for kind in (ref.XYZRGB, ref.XYZRGBMASK):
        want = ref.rows_text(kind, f, rgb, mask)
        got = capi.ascii_rows_host(kind, f, rgb, mask).tobytes()
        assert got == want, ref.first_difference(got, want)
    assert b" 4294967295 65535\n" in want and b" 4278190080 0\n" in want


def test_row_bounds_hold_on_the_longest_rows():
    capi = _capi()
    for kind, b in ref.BOUND.items():
        assert capi.ascii_row_bound(kind) == b
        f = np.full((3, ref.FLOATS[kind]), -1.1754944e-38, np.float32)  # 14 bytes per float
        rgb = np.full((3, 3), 255, np.uint8)
        mask = np.full(3, 65535, np.uint16)
        got = capi.ascii_rows_host(kind, f, rgb, mask).tobytes()
        assert got == ref.rows_text(kind, f, rgb, mask) and len(got) == 3 * b
    assert capi.ascii_row_bound(4) < 0 and capi.ascii_row_bound(-1) < 0


def test_capacity_contract_and_empty_input():
    capi = _capi()
    f, rgb, mask = ref.mixed_rows(ref.XYZRGBMASK, 300)
    want = ref.rows_text(ref.XYZRGBMASK, f, rgb, mask)
    out = np.full(len(want) + 8, 0xA5, np.uint8)
    with pytest.raises(capi.PcpError) as e:
        capi.ascii_rows_host(ref.XYZRGBMASK, f, rgb, mask, capacity=len(want) - 1, out=out)
    assert e.value.code == capi.PCP_ERR_RANGE and e.value.bytes == len(want)
    assert (out == 0xA5).all(), "a short capacity leaves the buffer untouched"
    got = capi.ascii_rows_host(ref.XYZRGBMASK, f, rgb, mask, capacity=len(want), out=out)  # the exact count suffices
    assert got.tobytes() == want and (out[len(want):] == 0xA5).all()
    for kind in ref.BOUND:
        assert capi.ascii_rows_host(kind, np.zeros((0, ref.FLOATS[kind]), np.float32), np.zeros((0, 3), np.uint8),
                                    np.zeros(0, np.uint16)).size == 0
    with pytest.raises(capi.PcpError) as e:
        capi.ascii_rows_host(ref.XYZRGB, f, None, None)  # the kind's colour array is missing
    assert e.value.code == capi.PCP_ERR_INVALID
    with pytest.raises(capi.PcpError) as e:
        capi.ascii_rows_host(ref.XYZI, ref.as_rows(f.reshape(-1), 4), capacity=-1)
    assert e.value.code == capi.PCP_ERR_INVALID


def test_symbols_are_declared_exported_and_bound_and_the_versions_stay():
    capi = _capi()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names and hasattr(lib, s), s
    for m in ("ascii_rows", "colour_compact_ascii", "mls_fetch_ascii"):
        assert callable(getattr(capi.Context, m)), m
    assert callable(capi.ascii_rows_host) and lib.pcp_abi_version() == 6


def test_header_with_the_new_declarations_is_plain_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "abi.c"
    calls = "\n".join(f"  (void){s};" for s in NEW)
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n' + calls +
                   "\n  return PCP_ABI_VERSION == 6 && PCP_K_COUNT == 13 && PCP_ROWS_POINTNORMAL == 3 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"), "-c", str(src),
                    "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)
