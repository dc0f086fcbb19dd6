"""SAMPLE_LOCAL_PLANE's sample table on the host (pcp_mls_local_plane_samples: no context, no GPU) against the fp32
restatement of the reference's loop, and the public constants that select it."""
import os
import re

import numpy as np
import pytest

import _mls_slp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("radius,step,count", [(0.05, 0.01, 79), (0.02, 0.004, 73), (0.1, 0.01, 313), (0.05, 0.005, 313)])
def test_table_counts_pinned(radius, step, count):
    u, v = ref.table(radius, step)
    assert len(u) == count


@pytest.mark.parametrize("radius,step", [(0.05, 0.01), (0.02, 0.004), (0.1, 0.01), (0.05, 0.005), (0.05, 0.003),
                                         (0.037, 0.0071), (1.0, 0.3), (0.05, 0.05), (0.05, 0.2)])
def test_library_table_equals_restatement_bit_for_bit(radius, step):
    from pointcloudprocessor_amd import capi

    u, v = capi.mls_local_plane_samples(radius, step)
    ru, rv = ref.table(radius, step)
    assert u.dtype == np.float32 and v.dtype == np.float32
    assert np.array_equal(u.view(np.uint32), ru.view(np.uint32))
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))


def test_reference_table_is_not_the_integer_lattice_nor_symmetric():
    from pointcloudprocessor_amd import capi

    u, v = capi.mls_local_plane_samples(0.05, 0.01)
    axis = sorted(set(v.tolist()))
    # 11 float values per axis from -0.050000001 to +0.049999997, an exact 0.0 among them
    full = sorted(set(ref.table(0.05, 0.01)[1].tolist()) | {float(np.float32(-0.05))})
    assert len(full) == 11 and 0.0 in axis
    assert np.float32(-0.05) not in set(v.tolist()) and np.float32(0.049999997) in set(v.tolist())
    pairs = set(zip(u.tolist(), v.tolist()))
    assert (0.0, float(np.float32(0.049999997))) in pairs
    assert (0.0, float(np.float32(-0.05))) not in pairs
    # 69 points of the integer lattice i^2 + j^2 < 25; the float steps admit 79
    assert len(pairs) == 79 and sum(1 for i in range(-5, 6) for j in range(-5, 6) if i * i + j * j < 25) == 69
    # emission order: u outer, v inner
    assert np.all(np.diff(u) >= 0)
    # a step that overshoots: (0.02, 0.004) ends each axis at 0.016
    u2, v2 = capi.mls_local_plane_samples(0.02, 0.004)
    assert np.isclose(u2.max(), 0.016, atol=1e-7) and np.isclose(v2.max(), 0.016, atol=1e-7)


def test_capacity_and_count_contract():
    import ctypes as C

    from pointcloudprocessor_amd import capi

    L = capi.load()
    n = C.c_int64(-1)
    assert L.pcp_mls_local_plane_samples(C.c_double(0.05), C.c_double(0.01), C.c_int64(0), None, None, C.byref(n)) == 0
    assert n.value == 79
    u = np.full(10, np.nan, np.float32)
    assert L.pcp_mls_local_plane_samples(C.c_double(0.05), C.c_double(0.01), C.c_int64(5), u.ctypes.data_as(C.c_void_p),
                                         None, C.byref(n)) == 0
    assert n.value == 79 and np.array_equal(u[:5], ref.table(0.05, 0.01)[0][:5]) and np.isnan(u[5:]).all()


@pytest.mark.parametrize("radius,step", [(0.0, 0.01), (0.05, 0.0), (-0.05, 0.01), (0.05, -0.01), (float("nan"), 0.01),
                                         (0.05, float("inf")), (float("inf"), 0.01), (0.05, 1e-60), (1.0, 1.0 / 600.0),
                                         (1e300, 1e299)])
def test_bad_arguments_are_refused(radius, step):
    import ctypes as C

    from pointcloudprocessor_amd import capi

    with pytest.raises(capi.PcpError) as e:
        capi.mls_local_plane_samples(radius, step)
    assert e.value.code == capi.PCP_ERR_INVALID
    n = C.c_int64()
    assert capi.load().pcp_mls_local_plane_samples(C.c_double(0.05), C.c_double(0.01), C.c_int64(-1), None, None,
                                                   C.byref(n)) == capi.PCP_ERR_INVALID


def test_ratio_bound_is_inclusive():
    from pointcloudprocessor_amd import capi

    u, _ = capi.mls_local_plane_samples(1.0, 1.0 / capi.MLS_SLP_MAX_RATIO)
    assert 0 < len(u) < 4 * capi.MLS_SLP_MAX_RATIO ** 2


def test_header_constants():
    from pointcloudprocessor_amd import capi

    header = open(os.path.join(ROOT, "include", "pcp_hip.h")).read()
    consts = dict(re.findall(r"#define (PCP_UPSAMPLING_[A-Z_]+) (\d+)", header))
    assert consts == {"PCP_UPSAMPLING_NONE": "0", "PCP_UPSAMPLING_SAMPLE_LOCAL_PLANE": "1",
                      "PCP_UPSAMPLING_VOXEL_GRID_DILATION": "3"}
    assert (capi.UPSAMPLING_NONE, capi.UPSAMPLING_SAMPLE_LOCAL_PLANE, capi.UPSAMPLING_VOXEL_GRID_DILATION) == (0, 1, 3)
    assert int(re.search(r"#define PCP_MLS_SLP_MAX_RATIO (\d+)", header).group(1)) == capi.MLS_SLP_MAX_RATIO
    assert "cloudSmooth.hpp enum order" not in header
    assert "pcp_set_mls_local_plane" in capi.declared_symbols()
    assert "pcp_mls_local_plane_samples" in capi.declared_symbols()
