"""Restatement of the planar facets ("Planar facets", FA2-FA7) in numpy / scipy, written from the rules and not from
the library's code: pairs from a k-d tree at 1.001 r filtered by the fp32 neighbour rule, FA3 and FA4 in numpy int64,
components from scipy.sparse.csgraph, labels by np.minimum.at, moments in Python integers, the plane from numpy.linalg.eigh.
It takes the normals and curvatures as inputs, so that a comparison does not depend on the last bit of an eigenvector."""
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

F32 = np.float32


def threshold_of(r) -> np.float32:
    """GN2: the largest float32 t with float64(t) <= float64(r)^2"""
    r2 = float(F32(r)) * float(F32(r))
    t = F32(r2)
    if float(t) > r2:
        t = np.nextafter(t, F32(0))
    return t


def link_constants(link_radius, angle_deg, plane_tol):
    c_q = math.ceil(math.cos(float(F32(angle_deg)) * (math.pi / 180.0)) * 2.0 ** 28)
    t_q = math.floor(float(F32(plane_tol)) * 2.0 ** 34)
    return threshold_of(link_radius), c_q, t_q


def facet_points(xyz, normal, curvature, max_curvature) -> np.ndarray:
    """FA2 (a valid normal: not (0, 0, 0), no component above 1 in magnitude, none a NaN)"""
    xyz = np.asarray(xyz, F32)
    normal = np.asarray(normal, F32)
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(xyz).all(axis=1)
        valid = (np.abs(normal) <= F32(1)).all(axis=1) & (normal != 0).any(axis=1)
        flat = np.asarray(curvature, F32) <= F32(max_curvature)
    return finite & valid & flat


def quantised_normals(normal) -> np.ndarray:
    """FA3: rint(n * 2^14), ties to even (the product is exact in float32)"""
    return np.rint(np.asarray(normal, F32) * F32(16384.0)).astype(np.int64)


def links(xyz, normal, is_facet_point, link_radius, angle_deg, plane_tol):
    """FA4: the linked pairs (i < j) as two index arrays"""
    t, c_q, t_q = link_constants(link_radius, angle_deg, plane_tol)
    idx = np.flatnonzero(is_facet_point)
    if len(idx) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    p = np.asarray(xyz, F32)[idx]
    pairs = cKDTree(p.astype(np.float64)).query_pairs(1.001 * float(F32(link_radius)), output_type="ndarray")
    a, b = pairs[:, 0], pairs[:, 1]
    d = (p[b] - p[a]).astype(F32)  # fl32(p_j - p_i)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32) + (d[:, 2] * d[:, 2]).astype(F32)
    near = d2 <= t
    a, b, d = a[near], b[near], d[near]
    nq = quantised_normals(np.asarray(normal, F32)[idx])
    na, nb = nq[a], nq[b]
    q = np.rint(d * F32(1048576.0)).astype(np.int64)  # gn::quantise: exact product, ties to even
    ok = np.abs((na * nb).sum(axis=1)) >= c_q
    ok &= (np.abs((na * q).sum(axis=1)) <= t_q) & (np.abs((nb * q).sum(axis=1)) <= t_q)
    return idx[a[ok]], idx[b[ok]]


def moments_fit(points: int, lo, hi) -> bool:
    extent = max(float(hi[a]) - float(lo[a]) for a in range(3))
    e = extent * 4096.0 + 1.0
    return float(points) * (e * e) < 2.0 ** 62


def facets(xyz, normal, curvature, link_radius=0.1, angle_deg=10.0, plane_tol=0.01, max_curvature=0.02, min_points=1000) -> dict:
    """dict(label (n,) int32, ids (F,) int32, rows (F, 10) int64, box (F, 6) float32, facet_points, components, facets)"""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    normal = np.ascontiguousarray(normal, F32).reshape(-1, 3)
    n = len(xyz)
    fp = facet_points(xyz, normal, curvature, max_curvature)
    i, j = links(xyz, normal, fp, link_radius, angle_deg, plane_tol)
    _, comp = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n)), directed=False)
    lowest = np.full(comp.max() + 1 if n else 0, n, np.int64)
    members = np.flatnonzero(fp)
    np.minimum.at(lowest, comp[members], members)
    label = np.full(n, -1, np.int64)
    label[members] = lowest[comp[members]]
    components = len(np.unique(label[members]))
    ids, counts = np.unique(label[members], return_counts=True)
    small = ids[counts < min_points]
    label[np.isin(label, small)] = -1
    ids = ids[counts >= min_points]
    rows = np.zeros((len(ids), 10), np.int64)
    box = np.zeros((len(ids), 6), F32)
    for r, fid in enumerate(ids):
        mem = xyz[label == fid]
        box[r, :3], box[r, 3:] = mem.min(axis=0), mem.max(axis=0)
        if not moments_fit(len(mem), box[r, :3], box[r, 3:]):
            raise OverflowError(f"facet {fid}")
        q = np.rint((mem - xyz[fid]).astype(F32) * F32(4096.0)).astype(np.int64)
        s = [len(mem)] + [sum(int(v) for v in q[:, a]) for a in range(3)]
        for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
            s.append(sum(int(u) * int(v) for u, v in zip(q[:, a], q[:, b])))
        rows[r] = s
    return dict(label=label.astype(np.int32), ids=ids.astype(np.int32), rows=rows, box=box, facet_points=int(fp.sum()),
                components=components, facets=len(ids))


def plane(root, row) -> np.ndarray:
    """FA7 by numpy.linalg.eigh: centroid (3), unit normal (3, largest component positive), rms (metres)"""
    n = int(row[0])
    s1 = np.array([int(v) for v in row[1:4]], np.float64)
    s2 = [float(int(v)) for v in row[4:10]]
    c = np.array([[s2[0], s2[1], s2[2]], [s2[1], s2[3], s2[4]], [s2[2], s2[4], s2[5]]]) - np.outer(s1, s1) / n
    w, v = np.linalg.eigh(c)
    nrm = v[:, 0]
    if nrm[np.argmax(np.abs(nrm))] < 0:
        nrm = -nrm
    centroid = np.asarray(root, F32).astype(np.float64) + (s1 / n) / 4096.0
    return np.concatenate([centroid, nrm, [math.sqrt(max(w[0], 0.0) / n) / 4096.0]])


def numpy_normals(xyz, radius):
    """A normal and a curvature per point from the neighbours within `radius` (float64 PCA; for the CPU suite, which has no
    estimate of the library's to feed): normal (n, 3) float32, curvature (n,) float32"""
    p = np.asarray(xyz, np.float64)
    tree = cKDTree(p)
    normal = np.zeros((len(p), 3), F32)
    curv = np.zeros(len(p), F32)
    for i, nb in enumerate(tree.query_ball_point(p, radius)):
        if len(nb) < 3:
            continue
        w, v = np.linalg.eigh(np.cov(p[nb].T, bias=True))
        normal[i] = v[:, 0]
        curv[i] = w[0] / max(w.sum(), 1e-300)
    return normal, curv
