"""The map comparison on the device ("Map comparison") against the restatement in _compare_ref.py and the host form:
integers, status and stats by equality, distance and lod by bytes; then the state rules of MC8, one assertion each."""
import numpy as np
import pytest

import _compare_ref as ref
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


def _run(ctx, c, normals="case", **over):
    xyz = c["xyz"]
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    ctx.compare_set_base(c["base"])
    kw = dict(c["kw"])
    kw.update(over)
    return ctx.compare(normals=c["normals"] if isinstance(normals, str) else normals, **kw)


@pytest.mark.parametrize("name", ref.CASES)
def test_device_equals_the_restatement_and_the_host_form(gpu_ctx_factory, name):
    c, want = ref.case_and_ref(name)
    got = _run(_ctx(gpu_ctx_factory), c)
    assert ref.same_bytes(got, want) is None, ref.same_bytes(got, want)
    host = _capi().compare_host(c["xyz"], c["normals"], c["base"], **c["kw"])
    assert ref.same_bytes(got, host) is None, ref.same_bytes(got, host)
    st = got["status"]
    assert got["stats"].tolist() == [(st != 0).sum(), (st >= 3).sum(), (st == 4).sum(), (st == 5).sum(), (st == 1).sum(), (st == 2).sum(),
                                     max(got["sums"][:, 0].max(), got["sums"][:, 4].max()), 0]


def test_bump_with_the_contexts_own_normals(gpu_ctx_factory):
    c, _ = ref.case_and_ref("bump")
    ctx = _ctx(gpu_ctx_factory)
    xyz = c["xyz"]
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    ctx.compare_set_base(c["base"])
    assert ctx.estimate_normals(0.05) > 5900
    nrm = ctx.normals_fetch()["normal"]
    own = ctx.compare(**c["kw"])
    given = ctx.compare(normals=nrm, **c["kw"])
    assert ref.same_bytes(own, given) is None, ref.same_bytes(own, given)
    want = ref.compare(xyz, nrm, c["base"], **c["kw"])
    assert ref.same_bytes(own, want) is None, ref.same_bytes(own, want)
    uv = c["uv"]
    inside = np.hypot(uv[:, 0] - 0.5, uv[:, 1] - 0.5) < 0.16
    assert (own["status"][inside] == 4).all() and (np.abs(own["distance"][inside].astype(np.float64) - 0.005) <= 0.0015).all()


@pytest.mark.parametrize("form", ["0", "1"])
def test_crowded_and_permuted_in_both_grid_forms(gpu_ctx_factory, monkeypatch, form):
    """The table of cell starts dense and sparse (PCP_GRID_SPARSE, read per call): the same bytes."""
    monkeypatch.setenv("PCP_GRID_SPARSE", form)
    ctx = _ctx(gpu_ctx_factory)
    c, want = ref.case_and_ref("crowded")
    got = _run(ctx, c)
    assert ref.same_bytes(got, want) is None, ref.same_bytes(got, want)
    shuffled, pa = ref.permute(c)
    again = _run(ctx, shuffled)
    for k in ("distance", "lod", "status", "sums", "direction"):
        assert again[k].tobytes() == want[k][pa].tobytes(), k
    assert np.array_equal(again["stats"], want["stats"])
    w = ref.wall(1500, 11)
    plain = _run(ctx, w)
    shuffled, pa = ref.permute(w)
    again = _run(ctx, shuffled)
    for k in ("distance", "lod", "status", "sums", "direction"):
        assert again[k].tobytes() == plain[k][pa].tobytes(), k
    assert ref.same_bytes(plain, _capi().compare_host(w["xyz"], w["normals"], w["base"], **w["kw"])) is None


def test_flip_on_the_device(gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    w = ref.wall(1500, 11)
    for kw in (dict(orient=tuple(np.array(w["kw"]["orient"]) - 4.0 * ref.E_N)), dict(orient_mode=2, orient=tuple(-ref.E_N)),
               dict(orient_mode=0)):
        got = _run(ctx, w, **kw)
        host = _capi().compare_host(w["xyz"], w["normals"], w["base"], **dict(w["kw"], **kw))
        assert ref.same_bytes(got, host) is None, (kw, ref.same_bytes(got, host))


def test_no_base_rows_and_a_base_far_away(gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    w = ref.wall(600, 13)
    for base in (np.zeros((0, 3), np.float32), w["base"] + np.float32(1.0)):
        c = dict(w, base=base)
        got = _run(ctx, c)
        assert ref.same_bytes(got, _capi().compare_host(c["xyz"], c["normals"], base, **c["kw"])) is None
        assert (got["status"] <= 1).all() and got["stats"][4] == got["stats"][0] > 500


def test_refusals_on_the_device(gpu_ctx_factory):
    capi = _capi()
    ctx = _ctx(gpu_ctx_factory)
    w = ref.wall(600, 13)
    for kw in (dict(radius=0.3, half_length=0.4), dict(min_points=1), dict(radius=0.004), dict(half_length=0.004), dict(reg_error=-1.0)):
        with pytest.raises(capi.PcpError) as e:
            _run(ctx, w, **kw)
        assert e.value.code == capi.PCP_ERR_INVALID, kw


# ---- MC8: state ----------------------------------------------------------------------------------------------------------------
def test_state_rules(gpu_ctx_factory):
    capi = _capi()
    ctx = gpu_ctx_factory()
    w = ref.wall(600, 13)
    xyz = w["xyz"]

    def refused(call, word):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_STATE and word in str(e.value), str(e.value)

    refused(lambda: ctx.compare(**w["kw"]), "no cloud")  # neither a cloud ...
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    refused(lambda: ctx.compare(normals=w["normals"], **w["kw"]), "pcp_compare_set_base")  # ... nor a base
    ctx.compare_set_base(w["base"])
    refused(lambda: ctx.compare(**w["kw"]), "pcp_estimate_normals")  # no normals
    refused(ctx.compare_fetch, "no result")  # a fetch before a result
    first = ctx.compare(normals=w["normals"], **w["kw"])
    assert ref.same_bytes(ctx.compare_fetch(), first, keys=("distance", "lod", "status", "sums", "direction")) is None
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    refused(ctx.compare_fetch, "no result")  # the result is dropped by an upload ...
    again = ctx.compare(normals=w["normals"], **w["kw"])  # ... and the base is kept
    assert ref.same_bytes(again, first) is None
    ctx.compare_set_base(w["base"] + np.float32(1.0))  # a second base replaces the first
    assert (ctx.compare(normals=w["normals"], **w["kw"])["status"] <= 1).all()
    ctx.compare_end()
    refused(ctx.compare_fetch, "no result")  # compare_end drops the result ...
    refused(lambda: ctx.compare(normals=w["normals"], **w["kw"]), "pcp_compare_set_base")  # ... and the base
    ctx.compare_end()  # (twice is fine)


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
    got = ctx.compare(radius=0.3, half_length=0.3, min_points=3)
    assert got["stats"][1] > 10000 and got["stats"][1] == (got["status"] >= 3).sum()
    after = ctx.normals_fetch()
    for k in normals:
        assert after[k].tobytes() == normals[k].tobytes(), k
    assert ctx.download_result_packed().tobytes() == packed.tobytes()
    again = ctx.colorize()
    assert again["rgb"].tobytes() == colour["rgb"].tobytes() and again["has"].tobytes() == colour["has"].tobytes()
