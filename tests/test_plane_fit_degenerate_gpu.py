"""Degenerate neighbourhoods through the real plane-fit kernels: k_gn_normals (pcp_estimate_normals) and k_mls_fit
(pcp_mls_process, orders 1 and 2) on one cloud of isolated clusters -- lines, exact lattices, duplicates, clusters of exactly
3, 5, 6 and 7 points, an isotropic lattice, needles, thin slabs -- about 1 m, 16 m and 300 m from the origin, in both grid forms.

Every cluster is at most 0.025 m across and 1 m from the next, so at radius 0.03 the neighbourhood of each of its points is
the cluster, in the normals (<= t) and in MLS (< r^2) alike.  The copies 300 m out are a cloud of their own: otherwise the
bounding box would decide the grid form for everything.

References: tests/_geometry_ref.py (integer moments, covariance, numpy.linalg.eigh) for the normals, the C oracle for MLS.
Where the eigenvector is not defined the tests assert what every right answer has in common (a unit vector of small residual
or an invalid point; finite rows; the query position kept) and write the order-2 displacements into
profiles/eigen33_selftest.md; they assert no agreement there, because the reference guarantees none."""
import numpy as np
import pytest

import _eigen33_ref as R
import _geometry_ref as gref
from test_mls_gpu import _compare

pytestmark = pytest.mark.gpu

RADIUS = 0.03
DIAMETER = 0.025

# class -> what the eigenvector is: "defined" (gap >= 1e-3: valid, the parity bars), "invalid" (every cross product exactly
# zero: no normal), "line" (a general fp32 line: valid, perpendicular to it), "either" (invalid, or a unit vector of small residual)
KIND = {"axis line": "invalid", "duplicates": "invalid", "(1,1,0) line": "either", "oblique line": "line",
        "axis plane lattice": "defined", "tilted plane lattice": "defined", "plane K=3": "defined", "plane K=5": "defined",
        "plane K=6": "defined", "plane K=7": "defined", "isotropic lattice": "either", "duplicates + 1": "either",
        "needle": "either", "thin slab": "defined"}
CLASSES = tuple(KIND)
_UV = np.array([(-1.0, -0.6), (1.0, -0.5), (0.1, 0.9), (0.5, 0.35), (-0.65, 0.45), (-0.2, -0.95), (0.8, 0.6)]) * 0.009


def _local(name, rng):
    """(points (K, 3) float64 about 0, direction or None): the cluster before it is moved to its place.  Coordinates that
    have to survive the move exactly are multiples of 2^-12 (the centres are multiples of 1/64; fp32 resolves 2^-15 at 300 m)."""
    q = 2.0 ** -12
    if name == "axis line":
        axis = int(rng.integers(0, 3))
        p = np.zeros((9, 3))
        p[:, axis] = np.arange(-4, 5) * 11 * q
        return p, np.eye(3)[axis]
    if name == "(1,1,0) line":
        t = np.arange(-4, 5) * 7 * q
        return np.stack([t, t, np.zeros(9)], 1), np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    if name == "oblique line":
        d = rng.uniform(0.25, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
        d /= np.linalg.norm(d)
        return np.linspace(-0.012, 0.012, 21)[:, None] * d, d
    if name == "axis plane lattice":
        i, j = np.meshgrid(np.arange(-2, 3), np.arange(-2, 3))
        return np.stack([i.ravel() * 16 * q, j.ravel() * 16 * q, np.zeros(25)], 1), None
    if name == "tilted plane lattice":
        i, j = np.meshgrid(np.arange(-2, 3), np.arange(-2, 3))
        a, b = np.array([12, 0, 6]) * q, np.array([0, 12, -9]) * q
        return i.ravel()[:, None] * a + j.ravel()[:, None] * b, None
    if name.startswith("plane K="):
        K = int(name[8:])
        Q = R._rotation(rng)
        return _UV[:K, :1] * Q[:, 0] + _UV[:K, 1:] * Q[:, 1], None
    if name == "isotropic lattice":
        g = np.arange(-1, 2) * 24 * q
        return np.stack(np.meshgrid(g, g, g), -1).reshape(-1, 3), None
    if name == "duplicates":
        return np.zeros((8, 3)), None
    if name == "duplicates + 1":
        return np.concatenate([np.zeros((8, 3)), [[16 * q, 12 * q, 20 * q]]]), None
    if name == "needle":
        Q = R._rotation(rng)
        return (np.linspace(-0.012, 0.012, 20)[:, None] * Q[:, 0] + rng.normal(0, 2e-4, (20, 1)) * Q[:, 1]
                + rng.normal(0, 2e-4, (20, 1)) * Q[:, 2]), Q[:, 0]
    if name == "thin slab":
        Q = R._rotation(rng)
        uvw = rng.uniform(-1, 1, (30, 3)) * [0.008, 0.008, 0.0002]
        return uvw @ Q.T, None
    raise KeyError(name)


def _build(bases, seed):
    """One shuffled cloud: every class five times at each base, the clusters on a 1 m lattice in x, y."""
    rng = np.random.default_rng(seed)
    pts, cls, cid, dirs = [], [], [], []
    for base in bases:
        k = 0
        for rep in range(5):
            for c, name in enumerate(CLASSES):
                p, d = _local(name, rng)
                centre = np.asarray(base, np.float64) + [k % 7, -(k // 7), 0.0]
                k += 1
                p = (centre + p).astype(np.float32)
                span = p.astype(np.float64)
                assert np.linalg.norm(span[:, None] - span[None], axis=2).max() <= DIAMETER, name
                pts.append(p)
                cls += [c] * len(p)
                cid += [len(dirs)] * len(p)
                dirs.append(np.zeros(3) if d is None else d)
    xyz, cls, cid = np.concatenate(pts), np.array(cls), np.array(cid)
    perm = rng.permutation(len(xyz))
    xyz, cls, cid = np.ascontiguousarray(xyz[perm]), cls[perm], cid[perm]
    size = np.bincount(cid)[cid]
    return dict(xyz=xyz, cls=cls, cid=cid, size=size, dirs=np.array(dirs)[cid], kind=np.array([KIND[CLASSES[c]] for c in cls]))


@pytest.fixture(scope="module")
def clouds(oracle):
    return _clouds(oracle)


def _clouds(oracle):
    """The two clouds with everything the references say about them, computed once: moments, covariance, eigh, and the
    oracle's MLS rows at orders 1 and 2."""
    out ={"near": _build([(1.0, 1.0, 1.0), (16.0, -16.0, 3.0)], 11), "far": _build([(300.0, -300.0, 100.0)], 12)}
    for c in out.values():
        xyz = c["xyz"]
        assert 800 <= len(xyz) <= 4000
        c["mom"] = gref.moments(RADIUS, xyz)
        assert np.array_equal(c["mom"][:, 0], c["size"])  # every neighbourhood is exactly its cluster
        c["C"] = gref.covariance(c["mom"])
        c["w"], c["v"] = np.linalg.eigh(c["C"])
        c["twin"] = gref.normals(c["mom"])
        c["mls"] = {}
        for order in (1, 2):
            op = oracle.default_mls_params()
            op.upsampling = 0
            op.polynomial_order = order
            op.threads = 8
            assert abs(op.search_radius - RADIUS) < 1e-12
            c["mls"][order] = oracle.mls(xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), op)
    return out


def _residual(C, w, n):
    """|C n - (n^T C n) n| / l2 per row, in long double"""
    Cl, nl = C.astype(R.LD), n.astype(R.LD)
    Cn = np.einsum("nab,nb->na", Cl, nl)
    r = Cn - (Cn * nl).sum(axis=1, keepdims=True) * nl
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.sqrt((r * r).sum(axis=1)) / w[:, 2].astype(R.LD)).astype(np.float64)


def _context(gpu_ctx_factory, monkeypatch, grid_form, xyz):
    monkeypatch.setenv("PCP_GRID_SPARSE", "1" if grid_form == "sparse" else "0")
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy())
    return ctx


@pytest.mark.parametrize("grid_form", ["dense", "sparse"])
@pytest.mark.parametrize("which", ["near", "far"])
def test_normals_of_degenerate_neighbourhoods(gpu_ctx_factory, clouds, which, grid_form, monkeypatch):
    c = clouds[which]
    ctx = _context(gpu_ctx_factory, monkeypatch, grid_form, c["xyz"])
    valid_count, mom = ctx.estimate_normals(RADIUS, want_moments=True)
    got = ctx.normals_fetch()
    assert mom.tobytes() == c["mom"].tobytes()
    assert np.array_equal(got["neighbours"], c["size"])
    nrm, curv, kind = got["normal"], got["curvature"], c["kind"]
    assert np.isfinite(nrm).all() and np.isfinite(curv).all()
    valid = nrm.any(axis=1)
    assert valid_count == int(valid.sum())
    assert not curv[~valid].any()
    # axis-parallel lines and duplicates: every cross product is exactly zero
    assert (kind == "invalid").sum() >= 80 and not valid[kind == "invalid"].any()
    # every valid point: a unit vector whose residual is that of the fp32-rounded eigh normal
    n = nrm.astype(np.float64)
    assert np.abs(np.linalg.norm(n[valid], axis=1) - 1.0).max() <= 1e-6
    res = _residual(c["C"], c["w"], n)
    res_eigh = _residual(c["C"], c["w"], c["v"][:, :, 0].astype(np.float32).astype(np.float64))
    bar = np.maximum(8.0 * res_eigh, 1e-6)
    over = valid & ~(res <= bar)
    print(which, grid_form, "valid", int(valid.sum()), "of", len(valid), "worst residual / bar", float((res[valid] / bar[valid]).max()))
    assert not over.any(), sorted({CLASSES[k] for k in c["cls"][over]})
    # defined planes: valid, and the existing parity bars against the eigh twin
    d = kind == "defined"
    assert d.sum() >= 300 and (c["twin"]["gap"][d] >= 1e-3).all() and c["twin"]["valid"][d].all()
    assert valid[d].all(), sorted({CLASSES[k] for k in c["cls"][d & ~valid]})
    t = c["twin"]["normal"][d]
    t = t * np.where((n[d] * t).sum(axis=1) < 0, -1.0, 1.0)[:, None]
    assert np.abs(n[d] - t).max() <= 1e-4
    cerr, ct = np.abs(curv[d].astype(np.float64) - c["twin"]["curvature"][d]), c["twin"]["curvature"][d]
    assert ((cerr <= 1e-4 * np.abs(ct)) | (cerr <= 1e-9)).all()
    # a general fp32 line: valid, the normal perpendicular to it (and otherwise arbitrary)
    ln = kind == "line"
    assert ln.sum() >= 60 and valid[ln].all()
    nd = np.abs((n[ln] * c["dirs"][ln]).sum(axis=1))
    nd_eigh = np.abs((c["v"][ln][:, :, 0] * c["dirs"][ln]).sum(axis=1))
    print(which, grid_form, "oblique lines: worst |n.d|", float(nd.max()), "eigh", float(nd_eigh.max()))
    assert (nd <= np.maximum(8.0 * nd_eigh, 1e-4)).all()
    # isotropic lattices, needles, (1,1,0) lines, duplicates + 1: invalid or under the residual rule above -- both occur nowhere wrong
    e = kind == "either"
    assert e.sum() >= 100


@pytest.mark.parametrize("grid_form", ["dense", "sparse"])
@pytest.mark.parametrize("which", ["near", "far"])
def test_mls_of_degenerate_neighbourhoods(gpu_ctx_factory, clouds, which, grid_form, monkeypatch):
    from pointcloudprocessor_amd import capi

    c = clouds[which]
    xyz, kind = c["xyz"], c["kind"]
    ctx = _context(gpu_ctx_factory, monkeypatch, grid_form, xyz)
    rows = []
    for order in (1, 2):
        mp = capi.default_mls_params()
        mp.upsampling = 0
        mp.polynomial_order = order
        got = ctx.mls_fetch(ctx.mls_process(mp))
        ref = c["mls"][order]
        assert np.array_equal(got["index"], ref["index"])
        assert len(got["index"]) == len(xyz)  # every cluster has 3 points or more
        idx = got["index"]
        for k in ("xyz", "normal", "curvature"):
            assert np.isfinite(got[k]).all(), (order, k)
        n = got["normal"].astype(np.float64)
        zero = ~got["normal"].any(axis=1)
        assert np.abs(np.linalg.norm(n[~zero], axis=1) - 1.0).max() <= 1e-6
        assert (got["curvature"] >= 0).all() and (got["curvature"] <= 1.0 / 3.0 + 1e-6).all()
        assert got["xyz"][zero].tobytes() == xyz[idx][zero].tobytes()  # no normal: the query position, bit for bit
        assert not got["curvature"][zero].any()
        move = np.linalg.norm(got["xyz"].astype(np.float64) - xyz[idx].astype(np.float64), axis=1)
        move_ref = np.linalg.norm(ref["xyz"].astype(np.float64) - xyz[idx].astype(np.float64), axis=1)
        if order == 1:
            # a projection onto a plane through the centroid of neighbours within R cannot move a point further than R
            assert move.max() <= RADIUS * (1 + 1e-6), move.max()
        # the classes with a defined plane, K = 3, 5, 6, 7 included: the parity bars of test_mls_gpu
        d = kind[idx] == "defined"
        assert d.sum() >= 300
        _compare({k: v[d] for k, v in got.items()}, {k: v[d] for k, v in ref.items()}, None)
        # exactly degenerate: no normal on the device, as in the oracle
        inv = kind[idx] == "invalid"
        assert zero[inv].all() and not ref["normal"][inv].any()
        if order == 2:
            for name in CLASSES:
                if KIND[name] in ("defined", "invalid"):
                    continue
                m = c["cls"][idx] == CLASSES.index(name)
                rows.append(f"| {which} | {grid_form} | {name} | {m.sum()} | {int(zero[m].sum())} | {int((~ref['normal'][m].any(axis=1)).sum())} | "
                            f"{R.fmt(float(move[m].max()))} | {R.fmt(float(move_ref[m].max()))} |")
        # two runs give the same bytes
        again = ctx.mls_fetch(ctx.mls_process(mp))
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), (order, k)
    head = ["| cloud | grid | class | rows | zero normal, device | zero normal, oracle | largest move, device [m] | largest move, oracle [m] |",
            "|---|---|---|---|---|---|---|---|"]
    print("\n".join(head + rows))
    R.write_block(f"stages {which} {grid_form}", "\n".join(head + rows))
