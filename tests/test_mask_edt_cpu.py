"""CPU suite of the mask distance maps (csrc/pcp_mask_edt.hpp through pcp_mask_edt_host: no context, no GPU) against the
brute-force restatement in _mask_edt_ref.py and against scipy.ndimage.distance_transform_edt, the function the reference's
preprocess() calls.  Every comparison is exact equality."""
import numpy as np
import pytest
import scipy.ndimage

import _mask_edt_ref as ref

NEW = ("pcp_mask_edt", "pcp_mask_edt_frames", "pcp_mask_edt_host")


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


def _check(mask, threshold=0):
    """host form == restatement (both outputs) == scipy (distance, where a background pixel exists)"""
    got = _capi().mask_edt_host(mask, threshold)
    want_d2, want_nearest = ref.edt(mask, threshold)
    h, w = mask.shape
    assert got["d2"].dtype == np.uint32 and got["d2"].shape == (h, w)
    assert got["nearest"].dtype == np.int32 and got["nearest"].shape == (h, w)
    assert np.array_equal(got["d2"], want_d2)
    assert np.array_equal(got["nearest"], want_nearest)
    fg = np.asarray(mask) > threshold
    if not fg.all():
        assert np.array_equal(np.sqrt(got["d2"].astype(np.float64)), scipy.ndimage.distance_transform_edt(fg))
        assert np.array_equal(got["nearest"][~fg], np.flatnonzero(~fg)), "a background pixel is its own nearest"
        assert not (got["d2"][fg] == 0).any() and not got["d2"][~fg].any()
    return got


def test_the_library_exports_the_entry_points():
    lib = _capi().load()
    for name in NEW:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("density", ref.DENSITIES)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_form_equals_the_restatement_and_scipy(shape, density):
    mask = ref.random_mask(shape, density, seed=1000 * shape[0] + shape[1])
    got = _check(mask)
    if density >= 1.0:
        assert (got["d2"] == ref.SENTINEL_D2).all() and (got["nearest"] == -1).all()
    if density == 0.0:
        assert not got["d2"].any()


@pytest.mark.parametrize("threshold", [0, 127, 254, 255])
def test_thresholds_on_random_bytes(threshold):
    mask = ref.byte_mask((45, 70), seed=7)
    got = _check(mask, threshold)
    assert int((got["d2"] == 0).sum()) == int((mask <= threshold).sum())
    if threshold == 255:
        assert not got["d2"].any(), "no byte exceeds 255: everything is background"


def test_ties_go_to_the_lowest_index():
    got = _check(ref.tie_mask())
    assert got["d2"][2, 2] == 4 and got["nearest"][2, 2] == 2
    # two background pixels of one column at the same distance: the upper row wins (the column stage's rule) ...
    col = np.full((5, 3), 9, np.uint8)
    col[0, 1] = col[4, 1] = 0
    got = _check(col)
    assert got["nearest"][2, 1] == 1 and got["d2"][2, 1] == 4
    # ... and of two columns at the same distance the one whose pixel has the lower index, left or right
    row = np.full((3, 5), 9, np.uint8)
    row[2, 0] = row[0, 4] = 0
    got = _check(row)
    assert got["nearest"][1, 2] == 4 and got["d2"][1, 2] == 5


def test_all_foreground_gives_the_sentinel():
    got = _capi().mask_edt_host(np.full((5, 7), 1, np.uint8))
    assert (got["d2"] == 0xFFFFFFFF).all() and (got["nearest"] == -1).all()
    got = _capi().mask_edt_host(np.full((5, 7), 200, np.uint8), 199)
    assert (got["d2"] == 0xFFFFFFFF).all()
    assert not _capi().mask_edt_host(np.full((5, 7), 200, np.uint8), 200)["d2"].any()


def test_a_row_stride_larger_than_the_width():
    big = ref.random_mask((33, 200), 0.5, seed=3)
    view = big[:, 5:134]  # 129 wide, rows 200 bytes apart
    assert view.strides == (200, 1)
    got = _capi().mask_edt_host(view)
    want = _capi().mask_edt_host(np.ascontiguousarray(view))
    assert np.array_equal(got["d2"], want["d2"]) and np.array_equal(got["nearest"], want["nearest"])
    assert np.array_equal(got["d2"], ref.edt(view)[0])


def test_outputs_are_nullable():
    import ctypes as C

    capi = _capi()
    mask = ref.random_mask((9, 11), 0.5, seed=5)
    d2 = np.empty((9, 11), np.uint32)
    nearest = np.empty((9, 11), np.int32)
    L = capi.load()
    args = (C.c_int32(11), C.c_int32(9), mask.ctypes.data_as(C.c_void_p), C.c_int64(11), C.c_int32(0))
    assert L.pcp_mask_edt_host(*args, d2.ctypes.data_as(C.c_void_p), None) == capi.PCP_OK
    assert L.pcp_mask_edt_host(*args, None, nearest.ctypes.data_as(C.c_void_p)) == capi.PCP_OK
    want = ref.edt(mask)
    assert np.array_equal(d2, want[0]) and np.array_equal(nearest, want[1])


def test_error_returns():
    import ctypes as C

    capi = _capi()
    L = capi.load()
    mask = np.zeros((4, 6), np.uint8)
    out = np.empty((4, 6), np.uint32)
    p, o = mask.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def call(w, h, ptr, stride, t):
        return L.pcp_mask_edt_host(C.c_int32(w), C.c_int32(h), ptr, C.c_int64(stride), C.c_int32(t), o, None)

    assert call(6, 4, p, 6, 0) == capi.PCP_OK
    assert call(6, 4, None, 6, 0) == capi.PCP_ERR_INVALID
    assert call(6, 4, p, 5, 0) == capi.PCP_ERR_INVALID and "stride" in L.pcp_last_error(None).decode()
    assert call(0, 4, p, 6, 0) == capi.PCP_ERR_INVALID
    assert call(6, 0, p, 6, 0) == capi.PCP_ERR_INVALID
    assert call(6, 4, p, 6, -1) == capi.PCP_ERR_INVALID
    assert call(6, 4, p, 6, 256) == capi.PCP_ERR_INVALID and "threshold" in L.pcp_last_error(None).decode()
    assert call(16385, 1, p, 16385, 0) == capi.PCP_ERR_RANGE and "16384" in L.pcp_last_error(None).decode()
    assert call(1, 16385, p, 1, 0) == capi.PCP_ERR_RANGE
    with pytest.raises(capi.PcpError) as e:
        capi.mask_edt_host(mask, 300)
    assert e.value.code == capi.PCP_ERR_INVALID


def test_the_widest_image_the_limit_allows():
    """W = 16384, the side at which a row's column words fill 64 KB: one background pixel at the far end, so that the
    left-most pixel's d2 is the largest a row can hold"""
    mask = np.full((2, 16384), 255, np.uint8)
    mask[1, 16383] = 0
    got = _capi().mask_edt_host(mask)
    x = np.arange(16384, dtype=np.int64)
    assert np.array_equal(got["d2"][1], ((16383 - x) ** 2).astype(np.uint32))
    assert np.array_equal(got["d2"][0], ((16383 - x) ** 2 + 1).astype(np.uint32))
    assert (got["nearest"] == 16384 + 16383).all()
