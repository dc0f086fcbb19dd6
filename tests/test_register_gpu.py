"""The map registration on the device ("Map registration") against the restatement in _register_ref.py and the host
form: the 60 words by equality, the transform, the log and the rows by bytes; then the state rules of RG1 and RG9, one
assertion each.  No case provokes a fault: every refusal is a check that returns before any launch."""
import functools

import numpy as np
import pytest

import _compare_ref as cref
import _register_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu


def _capi():
    from pointcloudprocessor_amd import capi

    return capi


_CTX = {}


def _ctx(make):
    """one context for the file; every test uploads the cloud and sets the base it needs"""
    if not _CTX:
        _CTX["ctx"] = make()
    return _CTX["ctx"]


def _load(ctx, c):
    xyz = c["xyz"]
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    ctx.compare_set_base(c["base"])


def _restated_sums(c):
    q, t = ref.identity()
    pivot, _ = ref.pivot_of(c["base"])
    return ref.evaluate(c["xyz"], c["normals"], c["base"], q, t, pivot, ref.params(**c["kw"]))


@functools.lru_cache(maxsize=None)
def _scene(name):
    return {"exact": ref.corner, "resampled": lambda: ref.corner(resampled=True), "wall": ref.wall_alone, "changed": ref.changed}[name]()


BOUNDARIES = ref.boundaries()


@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_boundary_sums(gpu_ctx_factory, name):
    c = BOUNDARIES[name]
    ctx = _ctx(gpu_ctx_factory)
    _load(ctx, c)
    got = ctx.compare_register_sums(normals=c["normals"], **c["kw"])
    assert [int(v) for v in got] == _restated_sums(c)
    host = _capi().compare_register_host(c["xyz"], c["normals"], c["base"], loop=False, **c["kw"])["sums"]
    assert np.array_equal(got, host)
    assert int(got[58]) == c["pairs"]


@pytest.mark.parametrize("name", ("exact", "resampled", "wall", "changed"))
def test_scene_sums(gpu_ctx_factory, name):
    c = _scene(name)
    ctx = _ctx(gpu_ctx_factory)
    _load(ctx, c)
    got = ctx.compare_register_sums(normals=c["normals"])
    assert [int(v) for v in got] == _restated_sums(c)
    assert np.array_equal(got, _capi().compare_register_host(c["xyz"], c["normals"], c["base"], loop=False)["sums"])
    assert int(got[58]) > 1900


def test_stride_three_and_the_lever_arm_on_the_device(gpu_ctx_factory):
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    c = ref.strided()
    _load(ctx, c)
    got = ctx.compare_register_sums(normals=c["normals"], **c["kw"])
    assert [int(v) for v in got] == _restated_sums(c) and 10 <= int(got[58]) <= 34
    c = ref.lever_beyond()
    _load(ctx, c)
    with pytest.raises(capi.PcpError) as e:  # (the box is judged on the host: nothing is launched)
        ctx.compare_register_sums(normals=c["normals"])
    assert e.value.code == capi.PCP_ERR_RANGE


@pytest.mark.parametrize("form", ["0", "1"])
def test_kernel_shapes_in_both_grid_forms(gpu_ctx_factory, monkeypatch, form):
    """The table of cell starts dense and sparse (PCP_GRID_SPARSE, read per call): the same words."""
    monkeypatch.setenv("PCP_GRID_SPARSE", form)
    ctx = _ctx(gpu_ctx_factory)
    # the grid's own formula puts every cluster into one cell of its own: 600 + 5 records in one cell, and so on
    assert ref.shape_occupancy(ref.shapes()) == list(ref.SHAPE_PLAN)
    assert max(nb + nm for nb, nm in ref.SHAPE_PLAN) > 512
    for c in (ref.shapes(), ref.one_cell_base()):
        _load(ctx, c)
        got = ctx.compare_register_sums(normals=c["normals"], **c["kw"])
        assert [int(v) for v in got] == _restated_sums(c)
        assert int(got[58]) == c["pairs"]
        # the order of the rows of either cloud does not show
        rng = np.random.default_rng(2)
        pa, pb = rng.permutation(len(c["xyz"])), rng.permutation(len(c["base"]))
        if len(np.unique(c["xyz"], axis=0)) == len(c["xyz"]):  # (the tie rule sees the order of equal points)
            _load(ctx, dict(xyz=c["xyz"][pa], base=c["base"][pb]))
            assert np.array_equal(ctx.compare_register_sums(normals=c["normals"][pa], **c["kw"]), got)


def test_own_normals_and_given_normals(gpu_ctx_factory):
    c = _scene("resampled")
    ctx = _ctx(gpu_ctx_factory)
    _load(ctx, c)
    assert ctx.estimate_normals(0.05) > 5900
    nrm = ctx.normals_fetch()["normal"]
    own = ctx.compare_register_sums()
    assert np.array_equal(own, ctx.compare_register_sums(normals=nrm))
    assert np.array_equal(own, _capi().compare_register_host(c["xyz"], nrm, c["base"], loop=False)["sums"])


@pytest.mark.parametrize("name", ("exact", "wall"))
def test_the_loop_equals_the_host_twin(gpu_ctx_factory, name):
    capi = _capi()
    c = _scene(name)
    ctx = _ctx(gpu_ctx_factory)
    _load(ctx, c)
    kw = dict(radius=0.03, half_length=0.05, min_points=5)
    before = ctx.compare(normals=c["normals"], **kw)
    got = ctx.compare_register(normals=c["normals"])
    host = capi.compare_register_host(c["xyz"], c["normals"], c["base"])
    want = ref.register(c["xyz"], c["normals"], c["base"])
    for other in (host, want):
        assert got["status"] == other["status"] == ref.CONVERGED and got["iterations"] == other["iterations"]
        assert got["T"].tobytes() == other["T"].tobytes() and got["log"].tobytes() == other["log"].tobytes()
    assert got["dof"] == (6 if name == "exact" else 3)
    state = ctx.compare_base_transform()
    assert state["T"].tobytes() == got["T"].tobytes() and state["ell"] == want["ell"] and state["pivot"].tobytes() == np.asarray(want["pivot"]).tobytes()
    # compare after the registration = compare after set_base with the rows the restatement transforms on the host
    after = ctx.compare(normals=c["normals"], **kw)
    ctx.compare_set_base(want["rows"])
    assert np.array_equal(ctx.compare_base_transform()["T"], np.eye(4))  # RG1: set_base resets T
    plain = ctx.compare(normals=c["normals"], **kw)
    assert cref.same_bytes(after, plain) is None, cref.same_bytes(after, plain)
    assert cref.same_bytes(after, before) is not None
    # 4 mm off, most of the corner was flagged; registered, the nominal share is
    print(name, "significant before", (before["status"] >= 4).mean(), "after", (after["status"] >= 4).mean())
    assert (after["status"] >= 4).mean() < 0.1 < (before["status"] >= 4).mean()


def test_a_set_transform_is_where_the_loop_starts(gpu_ctx_factory):
    capi = _capi()
    c = _scene("exact")
    ctx = _ctx(gpu_ctx_factory)
    _load(ctx, c)
    kw = dict(radius=0.03, half_length=0.05, min_points=5)
    original = ctx.compare(normals=c["normals"], **kw)
    ctx.compare_set_base_transform(c["T_true"])
    assert np.abs(ctx.compare_base_transform()["T"] - c["T_true"]).max() < 1e-12
    host = capi.compare_register_host(c["xyz"], c["normals"], c["base"], T_in=c["T_true"], loop=False)
    assert np.array_equal(ctx.compare_register_sums(normals=c["normals"]), host["sums"])
    moved = ctx.compare(normals=c["normals"], **kw)
    ctx.compare_set_base(host["rows"])
    assert cref.same_bytes(moved, ctx.compare(normals=c["normals"], **kw)) is None
    # RG1: the identity restores the original bytes
    ctx.compare_set_base(c["base"])
    ctx.compare_set_base_transform(c["T_true"])
    ctx.compare_set_base_transform(np.eye(4))
    assert cref.same_bytes(ctx.compare(normals=c["normals"], **kw), original) is None
    with pytest.raises(capi.PcpError) as e:
        ctx.compare_set_base_transform(np.diag([1.0, 1.0, -1.0, 1.0]))
    assert e.value.code == capi.PCP_ERR_INVALID


def test_too_few_pairs_leaves_the_base(gpu_ctx_factory):
    c = BOUNDARIES["trim_on_the_boundary"]
    ctx = _ctx(gpu_ctx_factory)
    _load(ctx, c)
    got = ctx.compare_register(normals=c["normals"], min_pairs=3, **c["kw"])
    assert got["status"] == ref.TOO_FEW_PAIRS and got["pairs"] == 2 and np.array_equal(got["T"], np.eye(4))


def test_refusals_on_the_device(gpu_ctx_factory):
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    c = BOUNDARIES["trim_on_the_boundary"]
    _load(ctx, c)
    for kw in (dict(match_radius=0.004), dict(match_radius=0.6), dict(max_plane_distance=0.06), dict(sample_stride=0), dict(max_iterations=0),
               dict(min_pairs=0), dict(tolerance=-1.0), dict(cond_tol=0.0)):
        for call in (ctx.compare_register, ctx.compare_register_sums):
            with pytest.raises(capi.PcpError) as e:
                call(normals=c["normals"], **kw)
            assert e.value.code == capi.PCP_ERR_INVALID, kw


# ---- RG1 / RG9: state ----------------------------------------------------------------------------------------------------------
def test_state_rules(gpu_ctx_factory):
    capi = _capi()
    ctx = gpu_ctx_factory()
    c = _scene("wall")
    xyz = c["xyz"]
    kw = dict(radius=0.03, half_length=0.05, min_points=5)

    def refused(call, word):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_STATE and word in str(e.value), str(e.value)

    refused(ctx.compare_register, "no cloud")  # neither a cloud ...
    refused(ctx.compare_register_sums, "no cloud")
    refused(ctx.compare_base_transform, "pcp_compare_set_base")
    refused(lambda: ctx.compare_set_base_transform(np.eye(4)), "pcp_compare_set_base")
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    refused(lambda: ctx.compare_register(normals=c["normals"]), "pcp_compare_set_base")  # ... nor a base
    ctx.compare_set_base(c["base"])
    refused(ctx.compare_register, "pcp_estimate_normals")  # no normals
    assert np.array_equal(ctx.compare_base_transform()["T"], np.eye(4))
    ctx.compare(normals=c["normals"], **kw)
    ctx.compare_register(normals=c["normals"])
    refused(ctx.compare_fetch, "no result")  # the base moved: the result is dropped
    moved = ctx.compare_base_transform()["T"]
    assert not np.array_equal(moved, np.eye(4))
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    assert np.array_equal(ctx.compare_base_transform()["T"], moved)  # the base and its transform stay across an upload
    ctx.compare_end()
    refused(ctx.compare_base_transform, "pcp_compare_set_base")  # compare_end drops everything


def test_nothing_else_moves(gpu_ctx_factory, small_scene):
    capi = _capi()
    s = small_scene
    ctx = gpu_ctx_factory()
    ctx.set_camera(cam_struct(capi, s["cam"]), capi.default_cull_params())
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.set_frames(s["poses"])
    for f, (im, mk) in enumerate(zip(s["images"], s["masks"])):
        ctx.upload_image(f, im)
        ctx.upload_mask(f, mk)
    colour = ctx.colorize()
    packed = ctx.download_result_packed()
    ctx.estimate_normals(0.5)
    normals = ctx.normals_fetch()
    xyz = np.stack([s["x"], s["y"], s["z"]], axis=1)
    base = xyz + np.float32(0.004) * normals["normal"]
    ctx.compare_set_base(base)
    got = ctx.compare_register(match_radius=0.3, max_plane_distance=0.1, sample_stride=2)
    assert got["pairs"] > 5000 and got["iterations"] >= 1
    after = ctx.normals_fetch()
    for k in normals:
        assert after[k].tobytes() == normals[k].tobytes(), k
    assert ctx.download_result_packed().tobytes() == packed.tobytes()
    again = ctx.colorize()
    assert again["rgb"].tobytes() == colour["rgb"].tobytes() and again["has"].tobytes() == colour["has"].tobytes()
