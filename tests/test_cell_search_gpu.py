"""The search the radius stages share (csrc/pcp_cell_search.hpp; DESIGN.md, "The cell-wave search") on one cloud built for the
walk's edges, through all three stages: local colour smoothing, the normals and the map comparison, each against its own
restatement, in both forms of the cell table and after a permutation of the input rows.

The cloud is the map of _compare_ref.crowded() with one all-NaN row appended.  At radius 0.06 its busiest cell holds several
work items of 64 queries, the last one partly filled; its busiest row of three cells is more than one LDS tile of 512 records;
a few hundred cells are occupied in a box of thousands, so rows are clipped at the box's faces; and in the comparison's joint
cloud the map items of the busiest cell end inside a cell whose tail is base records.  _case() recomputes those properties with
the grid's own formula and asserts them, so a later change to the case cannot empty this file silently."""
import math

import numpy as np
import pytest

import _compare_ref as cref
import _geometry_ref as gref
import _local_smooth_ref as sref

pytestmark = pytest.mark.gpu

F = np.float32
RADIUS = 0.06
QUERIES, TILE = 64, 512  # kCellQ, kCellTile
FORMS = ("unset", "0", "1")  # PCP_GRID_SPARSE: the library's choice (dense here), dense, sparse


def grid_of(pts, radius):
    """build_radius_grid's grid over finite float32 rows: (cell edge, (nx, ny, nz), per-row (ix, iy, iz))."""
    pts = np.asarray(pts, F)
    mn, mx = pts.min(axis=0), pts.max(axis=0)
    ext = (mx - mn).astype(F)
    vol = float(np.prod(np.maximum(ext.astype(np.float64), 1e-3)))
    by_density = F(np.cbrt(vol / (8.0 * len(pts))))
    cell = max(F(F(radius) * F(1.001)), by_density)
    inv = F(1.0) / cell
    dims = np.floor(ext * inv).astype(np.int64) + 1
    idx = np.clip(np.floor(((pts - mn).astype(F) * inv).astype(F)).astype(np.int64), 0, dims - 1)
    return float(cell), dims, idx


def occupancy(pts, radius):
    """dict(cell, cells = occupied cells, busiest_cell = its records, busiest_row = most records in three cells along x,
    where = the busiest cell's rows)."""
    cell, dims, idx = grid_of(pts, radius)
    ids = (idx[:, 2] * dims[1] + idx[:, 1]) * dims[0] + idx[:, 0]
    cells, counts = np.unique(ids, return_counts=True)
    count_of = dict(zip(cells.tolist(), counts.tolist()))
    busiest = int(cells[np.argmax(counts)])
    row = 0
    for c in cells.tolist():  # the run of the cells x - 1 .. x + 1 of a row, clipped at the faces
        x = c % int(dims[0])
        row = max(row, sum(count_of.get(c + d, 0) for d in (-1, 0, 1) if 0 <= x + d < dims[0]))
    return dict(cell=cell, dims=dims, cells=len(cells), busiest_cell=int(counts.max()), busiest_row=row, where=ids == busiest)


_CASE = {}


def _case():
    """The cloud, its inputs and the three restatements' results: computed once, shared among the tests, left unchanged."""
    if _CASE:
        return _CASE
    c = cref.crowded()
    nan_row = np.full((1, 3), np.nan, F)
    xyz = np.concatenate([c["xyz"], nan_row])
    normals = np.concatenate([c["normals"], np.array([[0.0, 0.0, 1.0]], F)])
    words = np.random.default_rng(17).integers(0, 1 << 25, len(xyz), dtype=np.uint32)  # colours and a random has bit
    words[::7] = 0
    n = len(xyz)
    assert n == 801 and not np.isfinite(xyz[-1]).any() and np.isfinite(xyz[:-1]).all()
    # ---- the properties this file is about, with the grid's formula ----
    own = occupancy(xyz[:-1], RADIUS)
    assert abs(own["cell"] - 0.06006) < 1e-6
    assert own["busiest_cell"] > QUERIES and own["busiest_cell"] % QUERIES != 0  # several work items, the last partly filled
    assert own["busiest_row"] > TILE  # a row of more than one tile
    assert own["cells"] < int(np.prod(own["dims"])) and (own["dims"] > 3).all()  # a sparse frame: rows end at the box's faces
    assert (own["busiest_cell"], math.ceil(own["busiest_cell"] / QUERIES), own["busiest_row"], own["cells"]) == (501, 8, 566, 199)
    s = float(cref.search_radius(0.03, 0.05))
    assert not c["kw"] and abs(s - 0.0583) < 1e-4  # the case's own keywords: the defaults
    joint = occupancy(np.concatenate([xyz[:-1], c["base"]]), s)
    map_rows = int(joint["where"][: n - 1].sum())
    assert joint["busiest_cell"] > TILE and joint["busiest_row"] > TILE
    assert QUERIES < map_rows < joint["busiest_cell"] and map_rows % QUERIES != 0  # the last map item ends among base records
    assert (joint["busiest_cell"], joint["busiest_row"]) == (636, 848)
    # ---- the restatements ----
    mom = gref.moments(RADIUS, xyz)
    twin = gref.normals(mom)
    _CASE.update(xyz=xyz, normals=normals, base=c["base"], kw=c["kw"], words=words,
                 perm=np.random.default_rng(23).permutation(n), base_perm=np.random.default_rng(29).permutation(len(c["base"])),
                 smooth=sref.smooth_local(xyz[:, 0], xyz[:, 1], xyz[:, 2], words, RADIUS), moments=mom, twin=twin,
                 compare=cref.compare(xyz, normals, c["base"], **c["kw"]))
    for v in _CASE.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return _CASE


_CTX = {}


def _ctx(make, monkeypatch, form, xyz):
    """one context for the file, the cloud uploaded, the form of the cell table set for the calls that follow"""
    if form == "unset":
        monkeypatch.delenv("PCP_GRID_SPARSE", raising=False)
    else:
        monkeypatch.setenv("PCP_GRID_SPARSE", form)
    if not _CTX:
        _CTX["ctx"] = make()
    ctx = _CTX["ctx"]
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    return ctx


def test_the_case_reaches_the_walks_edges():
    c = _case()
    assert c["twin"]["valid"].sum() > 600 and not c["twin"]["valid"][-1]
    assert (c["compare"]["status"] >= 3).sum() > 300 and c["compare"]["stats"][6] > QUERIES


@pytest.mark.parametrize("form", FORMS)
def test_smoothing(gpu_ctx_factory, monkeypatch, form):
    c = _case()
    xyz, words, want, p = c["xyz"], c["words"], c["smooth"], c["perm"]
    got, has = _ctx(gpu_ctx_factory, monkeypatch, form, xyz).colour_smooth_local_packed(RADIUS, words)
    assert got.tobytes() == want.tobytes()
    assert has == int(((want >> 24) & 1).sum())
    assert got[-1] == words[-1]  # the NaN row keeps its word, has bit and all
    again, has_again = _ctx(gpu_ctx_factory, monkeypatch, form, xyz[p]).colour_smooth_local_packed(RADIUS, words[p])
    assert again.tobytes() == want[p].tobytes() and has_again == has


_NORMALS = {}


@pytest.mark.parametrize("form", FORMS)
def test_normals(gpu_ctx_factory, monkeypatch, form):
    """The moments are the search's result and are equal by bytes.  The normal is the finish of pcp_eigen33.hpp on those
    moments, compared with numpy's eigh of the same covariance at the bar test_geometry_gpu.py holds it to, and equal by bytes
    between the forms of the table and under the permutation."""
    c = _case()
    xyz, mom, twin, p = c["xyz"], c["moments"], c["twin"], c["perm"]
    ctx = _ctx(gpu_ctx_factory, monkeypatch, form, xyz)
    valid, got = ctx.estimate_normals(RADIUS, want_moments=True)
    out = ctx.normals_fetch()
    assert got.tobytes() == mom.tobytes()
    assert np.array_equal(out["neighbours"], mom[:, 0].astype(np.int32))
    assert valid == int(twin["valid"].sum()) and np.array_equal(out["normal"].any(axis=1), twin["valid"])
    assert not out["curvature"][~twin["valid"]].any()
    assert not out["normal"][-1].any() and out["curvature"][-1] == 0 and out["neighbours"][-1] == 0 and not got[-1].any()  # the NaN row
    check = twin["valid"] & (twin["gap"] >= 1e-3)  # (below that gap the eigenvector itself is ill-conditioned)
    print("valid", valid, "checked", int(check.sum()), "smallest eigen-gap", float(twin["gap"][twin["valid"]].min()))
    assert check.sum() >= 0.99 * twin["valid"].sum()
    n, t = out["normal"][check].astype(np.float64), twin["normal"][check]
    err = np.abs(n - t * np.sign((n * t).sum(axis=1))[:, None]).max()
    print("largest component error", float(err))
    assert err <= 1e-4
    first = _NORMALS.setdefault("out", out)  # whichever form ran first: the others give its bytes
    for k in ("normal", "curvature", "neighbours"):
        assert out[k].tobytes() == first[k].tobytes(), k
    ctx = _ctx(gpu_ctx_factory, monkeypatch, form, xyz[p])
    valid_again, got_again = ctx.estimate_normals(RADIUS, want_moments=True)
    again = ctx.normals_fetch()
    assert valid_again == valid and got_again.tobytes() == mom[p].tobytes()
    for k in ("normal", "curvature", "neighbours"):
        assert again[k].tobytes() == out[k][p].tobytes(), k


@pytest.mark.parametrize("form", FORMS)
def test_comparison(gpu_ctx_factory, monkeypatch, form):
    c = _case()
    xyz, nrm, base, want, p, pb = c["xyz"], c["normals"], c["base"], c["compare"], c["perm"], c["base_perm"]
    ctx = _ctx(gpu_ctx_factory, monkeypatch, form, xyz)
    ctx.compare_set_base(base)
    got = ctx.compare(normals=nrm, **c["kw"])
    assert cref.same_bytes(got, want) is None, cref.same_bytes(got, want)
    assert got["status"][-1] == 0 and got["distance"][-1] == 0 and got["lod"][-1] == 0 and not got["sums"][-1].any()  # the NaN row
    ctx = _ctx(gpu_ctx_factory, monkeypatch, form, xyz[p])
    ctx.compare_set_base(base[pb])
    again = ctx.compare(normals=nrm[p], **c["kw"])
    for k in ("distance", "lod", "status", "sums", "direction"):
        assert again[k].tobytes() == want[k][p].tobytes(), k
    assert np.array_equal(again["stats"], want["stats"])
