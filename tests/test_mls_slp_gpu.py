"""SAMPLE_LOCAL_PLANE upsampling on the device (pcp_mls_process / pcp_cloud_smooth with upsampling 1) against the numpy
restatement (tests/_mls_slp_ref.py on oracle.np_oracle.mls_results), the chain against its composition, degenerate
planes, the size limit, the entry points that refuse it, and the context's other modes after it.
Bars as tests/test_mls_gpu.py (Appendix A9), normals compared ORIENTED: each twin plane takes the sign the device's own
fit chose (read from a NONE run of the same context), since a flipped plane mirrors the whole disk."""
import numpy as np
import pytest

import _mls_slp_ref as ref
from test_mls_gpu import _patches

pytestmark = pytest.mark.gpu

R = 0.03


def _params(upsampling, order=2):
    from pointcloudprocessor_amd import capi

    mp = capi.default_mls_params()
    mp.upsampling = upsampling
    mp.polynomial_order = order
    return mp


def _flips(none, results):
    """flips[i]: the twin's plane of point i points against the device's (the NONE normal has a positive dot product
    with the plane normal that produced it)."""
    flips = np.zeros(len(results), bool)
    for row, i in enumerate(none["index"]):
        flips[i] = float(np.dot(none["normal"][row].astype(np.float64), results[i]["normal"])) < 0.0
    return flips


@pytest.mark.parametrize("order", [0, 1, 2])
def test_slp_matches_twin(gpu_ctx_factory, order):
    from oracle import np_oracle

    x, y, z = _patches(seed=5, n=450)
    radius, step = 0.04, 0.013  # not the reference's values; the step does not divide the radius
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    ctx.set_mls_local_plane(radius, step)
    none = ctx.mls_fetch(ctx.mls_process(_params(0, order)))
    m = ctx.mls_process(_params(1, order))
    got = ctx.mls_fetch(m)
    tu, _ = ref.table(radius, step)
    T = len(tu)
    # exact: rows = table x fitted, each fitted index T times in ascending order
    assert m == T * len(none["index"])
    assert np.array_equal(got["index"], np.repeat(none["index"], T))
    res = np_oracle.mls_results(x, y, z, R, order)
    assert np.array_equal(np.array([i for i, r in enumerate(res) if r is not None]), none["index"])
    Ks = np.array([res[i]["K"] for i in none["index"]])
    assert (Ks < 6).any() and (Ks >= 6).any()  # clusters with 3 <= K < 6 and surfaces
    want = ref.emit(res, radius, step, order, _flips(none, res))
    assert np.array_equal(want["index"], got["index"])
    d = np.abs(got["xyz"].astype(np.float64) - want["xyz"].astype(np.float64))
    assert d.max() <= 1e-4 * R, d.max()
    dn = np.abs(got["normal"].astype(np.float64) - want["normal"].astype(np.float64))
    assert dn.max() <= 1e-4, dn.max()
    np.testing.assert_allclose(got["curvature"], want["curvature"], rtol=1e-4, atol=1e-9)
    if order == 2:  # the polynomial moved the samples off the plane somewhere
        flat = ref.emit(res, radius, step, 1, _flips(none, res))
        assert np.abs(flat["xyz"].astype(np.float64) - want["xyz"]).max() > 1e-4


def test_reference_defaults_from_create(gpu_ctx_factory):
    x, y, z = _patches(seed=9, n=300)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    fitted = ctx.mls_process(_params(0))
    assert ctx.mls_process(_params(1)) == 79 * fitted


def _chain_cloud(seed=41, n=4000):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.15, 0.15, (n, 2))
    zz = 0.6 * a[:, 0] ** 2 + 0.3 * a[:, 0] * a[:, 1] + rng.normal(0, 8e-4, n)
    pts = np.stack([a[:, 0] - 3.0, a[:, 1] + 1.0, zz + 1.2], 1)
    pts = np.concatenate([pts, rng.uniform(-0.15, 0.15, (40, 3)) + [-3.0, 1.0, 1.3]]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    return pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()


def test_chain_equals_its_composition(gpu_ctx_factory, oracle):
    """pcp_cloud_smooth(SLP) = oracle SOR on the input, then the device's SLP rows on an UPLOAD of the survivors, then
    oracle SOR on those rows: keep flags exact, rows bit for bit."""
    x, y, z = _chain_cloud()
    radius, step = 0.02, 0.004
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    ctx.set_mls_local_plane(radius, step)
    m = ctx.cloud_smooth(_params(1))
    got = ctx.mls_fetch(m)
    keep1, _ = oracle.sor(x, y, z, 60, 0.7, threads=8)
    idx1 = np.nonzero(keep1)[0]
    assert len(idx1) < len(x)
    ctx1 = gpu_ctx_factory()
    ctx1.upload_cloud(x[idx1], y[idx1], z[idx1])
    ctx1.set_mls_local_plane(radius, step)
    rows = ctx1.mls_fetch(ctx1.mls_process(_params(1)))
    assert len(rows["index"]) == 73 * len(np.unique(rows["index"]))
    keep2, _ = oracle.sor(rows["xyz"][:, 0].copy(), rows["xyz"][:, 1].copy(), rows["xyz"][:, 2].copy(), 60, 0.7, threads=8)
    k2 = np.nonzero(keep2)[0]
    assert 0 < len(k2) < len(rows["index"])
    assert m == len(k2)
    assert np.array_equal(got["index"], idx1[rows["index"][k2]])
    for k in ("xyz", "normal", "curvature"):
        assert np.array_equal(got[k].view(np.uint32), rows[k][k2].view(np.uint32)), k


def test_degenerate_planes_give_finite_rows(gpu_ctx_factory):
    """An exact-duplicate cluster (zero covariance: no plane) emits the NONE row of each of its points -- the point
    itself, zero normal, zero curvature -- once per sample; collinear points emit finite rows; nothing is NaN."""
    rng = np.random.default_rng(3)
    dup = np.repeat(np.array([[1.0, 2.0, 3.0]]), 5, axis=0)
    line = np.stack([np.linspace(0, 0.02, 6) + 5.0, np.full(6, -1.0), np.full(6, 0.5)], 1)
    a = rng.uniform(-0.05, 0.05, (300, 2))
    plane = np.stack([a[:, 0] - 2.0, a[:, 1], 0.1 * a[:, 0]], 1)
    pts = np.concatenate([dup, line, plane]).astype(np.float32)
    x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    none = ctx.mls_fetch(ctx.mls_process(_params(0)))
    got = ctx.mls_fetch(ctx.mls_process(_params(1)))
    assert len(got["index"]) == 79 * len(none["index"])
    for k in ("xyz", "normal", "curvature"):
        assert np.isfinite(got[k]).all(), k
    invalid = none["index"][np.all(none["normal"] == 0, axis=1)]
    assert set(range(5)) <= set(invalid.tolist())  # the duplicates have no plane
    for i in invalid:
        sel = got["index"] == i
        assert sel.sum() == 79
        assert np.array_equal(got["xyz"][sel], np.repeat(pts[i][None, :], 79, axis=0))
        assert not got["normal"][sel].any() and not got["curvature"][sel].any()
    line_rows = np.isin(got["index"], np.arange(5, 11))
    assert line_rows.sum() == 79 * 6 and np.isfinite(got["xyz"][line_rows]).all()
    # the whole chain over such a cloud stays finite as well
    got2 = ctx.mls_fetch(ctx.cloud_smooth(_params(1)))
    assert all(np.isfinite(got2[k]).all() for k in ("xyz", "normal", "curvature"))


def test_rows_beyond_one_result_fail_fast_without_allocating(gpu_ctx_factory):
    import time

    import torch

    from pointcloudprocessor_amd import capi

    rng = np.random.default_rng(8)
    a = rng.uniform(-0.4, 0.4, (8000, 2))  # rows ~6.6e9, and > 2^31 after the chain's first filter too
    pts = np.stack([a[:, 0], a[:, 1], 0.05 * a[:, 1]], 1).astype(np.float32)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
    step = 0.05 / capi.MLS_SLP_MAX_RATIO
    ctx.set_mls_local_plane(0.05, step)
    T = len(capi.mls_local_plane_samples(0.05, step)[0])
    fitted = ctx.mls_process(_params(0))
    assert T * fitted >= 2 ** 31
    free0 = torch.cuda.mem_get_info(0)[0]
    t0 = time.perf_counter()
    for call in (ctx.mls_process, ctx.cloud_smooth):
        with pytest.raises(capi.PcpError) as e:
            call(_params(1))
        assert e.value.code == capi.PCP_ERR_NOMEM
        assert "rows" in str(e.value) and str(T) in str(e.value)
    assert time.perf_counter() - t0 < 20.0
    assert torch.cuda.mem_get_info(0)[0] > free0 - (2 << 30)  # the rows would take ~80 GB


def test_refusing_entry_points_and_bad_settings(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi, pipeline

    x, y, z = _patches(seed=2, n=200)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    mp = _params(1)
    for call in (lambda: ctx.mls_process_shard(mp, 0, len(x)), lambda: ctx.mls_process_slab(mp, 0, 2),
                 lambda: ctx.mls_stream_begin(mp, 1 << 20), lambda: ctx.cloud_smooth_stream_begin(mp, 1 << 20)):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_INVALID and "SAMPLE_LOCAL_PLANE" in str(e.value)
    for r, s in ((0.05, 0.0), (0.0, 0.01), (float("nan"), 0.01), (1.0, 1e-4)):
        with pytest.raises(capi.PcpError) as e:
            ctx.set_mls_local_plane(r, s)
        assert e.value.code == capi.PCP_ERR_INVALID
    fitted = ctx.mls_process(_params(0))
    assert ctx.mls_process(mp) == 79 * fitted  # the refused settings left the defaults
    with pytest.raises(ValueError):
        pipeline.CloudSmooth(pipeline.HipEngine.__new__(pipeline.HipEngine), mp).process_sharded(len(x), 0, 2)


def test_other_modes_unchanged_after_slp(gpu_ctx_factory):
    x, y, z = _patches(seed=4, n=600)
    vgd = _params(3)
    vgd.vgd_voxel_size = 0.003
    vgd.vgd_iterations = 1
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    ctx.set_mls_local_plane(0.03, 0.007)
    ctx.mls_process(_params(1))
    ctx.cloud_smooth(_params(1))
    after = [ctx.mls_fetch(ctx.mls_process(_params(0))), ctx.mls_fetch(ctx.mls_process(vgd)),
             ctx.mls_fetch(ctx.cloud_smooth(_params(0))), ctx.mls_fetch(ctx.cloud_smooth(vgd))]
    fresh = gpu_ctx_factory()
    fresh.upload_cloud(x, y, z)
    before = [fresh.mls_fetch(fresh.mls_process(_params(0))), fresh.mls_fetch(fresh.mls_process(vgd)),
              fresh.mls_fetch(fresh.cloud_smooth(_params(0))), fresh.mls_fetch(fresh.cloud_smooth(vgd))]
    for a, b in zip(after, before):
        for k in ("index", "xyz", "normal", "curvature"):
            assert np.array_equal(a[k], b[k]), k


def test_pipeline_local_plane_option(gpu_ctx_factory):
    from pointcloudprocessor_amd import pipeline

    x, y, z = _patches(seed=6, n=300)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    eng = pipeline.HipEngine.__new__(pipeline.HipEngine)
    eng.ctx = ctx
    fitted = ctx.mls_process(_params(0))
    out = pipeline.CloudSmooth(eng, _params(1), local_plane=(0.02, 0.004)).process(with_outlier_removal=False)
    assert len(out["index"]) == 73 * fitted


def test_chain_refuses_rows_spanning_too_far(gpu_ctx_factory):
    """The trailing outlier removal's grid must span every row; rows spread over kilometres would force its cells far
    beyond the disks' spacing and its cost without bound: the chain refuses them (PCP_ERR_RANGE) before that filter,
    while MLS alone still emits them, and the same clusters a few metres apart run."""
    import time

    from pointcloudprocessor_amd import capi

    rng = np.random.default_rng(12)

    def clusters(spread):
        out = []
        for c in ([0.0, 0.0, 0.0], [spread, 0.0, 0.0], [0.0, spread, 0.0], [0.0, 0.0, spread]):
            a = rng.uniform(-0.06, 0.06, (400, 2))
            out.append(np.stack([a[:, 0], a[:, 1], 0.2 * a[:, 0] + rng.normal(0, 5e-4, 400)], 1) + c)
        p = np.concatenate(out).astype(np.float32)
        return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()

    ctx = gpu_ctx_factory()
    ctx.upload_cloud(*clusters(3000.0))
    t0 = time.perf_counter()
    with pytest.raises(capi.PcpError) as e:
        ctx.cloud_smooth(_params(1))
    assert e.value.code == capi.PCP_ERR_RANGE and "SAMPLE_LOCAL_PLANE" in str(e.value)
    assert time.perf_counter() - t0 < 20.0
    assert ctx.mls_process(_params(1)) > 0
    near = gpu_ctx_factory()
    near.upload_cloud(*clusters(3.0))
    assert near.cloud_smooth(_params(1)) > 0


def test_chain_refuses_more_rows_than_its_filter_takes(gpu_ctx_factory):
    """More than 2^24 rows: the chain refuses them (PCP_ERR_RANGE) before its trailing outlier removal, whose cost grows with
    rows x strays; MLS alone emits them."""
    import time

    from pointcloudprocessor_amd import capi

    rng = np.random.default_rng(21)
    a = rng.uniform(-0.4, 0.4, (5000, 2))
    pts = np.stack([a[:, 0], a[:, 1], 0.05 * a[:, 0] + rng.normal(0, 5e-4, 5000)], 1).astype(np.float32)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
    ctx.set_mls_local_plane(0.05, 0.05 / 40)
    assert ctx.mls_process(_params(1)) > 2 ** 24 * 1.2
    t0 = time.perf_counter()
    with pytest.raises(capi.PcpError) as e:
        ctx.cloud_smooth(_params(1))
    assert e.value.code == capi.PCP_ERR_RANGE and "exceed" in str(e.value)
    assert time.perf_counter() - t0 < 20.0
