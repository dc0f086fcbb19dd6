"""Restatement of the geometry maps ("Geometry maps") in numpy + scipy: the moments of GN2-GN5 in integer
arithmetic, normals by numpy.linalg.eigh of the same covariance, and the per-pixel reduction of GM2 as a lexsort."""
import numpy as np
from scipy.spatial import cKDTree

Q = 1048576.0  # GN3: 2^20 quanta per metre


def threshold(radius: float) -> np.float32:
    """GN2: the largest float t with (double)t <= (double)r^2, r the fp32 radius."""
    r = float(np.float32(radius))
    t = np.float32(r * r)
    if float(t) > r * r:
        t = np.nextafter(t, np.float32(0.0))
    return t


def dirty_cloud(xyz: np.ndarray) -> np.ndarray:
    """A copy with 300 exact duplicates appended and two points made non-finite."""
    rng = np.random.default_rng(41)
    out = np.concatenate([xyz, xyz[rng.choice(len(xyz), 300, replace=False)]]).copy()
    out[17, 1] = np.nan
    out[len(xyz) + 5, 2] = np.inf
    return out


def moments(radius: float, xyz: np.ndarray) -> np.ndarray:
    """(n, 10) int64: n S1x S1y S1z S2xx xy xz yy yz zz per point; zeros for a non-finite point (GN1)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    out = np.zeros((n, 10), np.int64)
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    if len(fin) == 0:
        return out
    p = xyz[fin]
    t = threshold(radius)
    # candidates from the tree at a slightly larger radius, then the fp32 rule decides
    pairs = cKDTree(p.astype(np.float64)).query_pairs(float(np.float32(radius)) * 1.001, output_type="ndarray")
    me = np.arange(len(p), dtype=np.int64)
    i = np.concatenate([pairs[:, 0], pairs[:, 1], me])
    j = np.concatenate([pairs[:, 1], pairs[:, 0], me])
    d = p[j] - p[i]  # fp32, per component
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    d2 = (dx * dx + dy * dy) + dz * dz  # fp32, every operation rounded on its own
    assert d2.dtype == np.float32
    keep = d2 <= t
    i, d = i[keep], d[keep]
    q = np.rint(d.astype(np.float64) * Q).astype(np.int64)  # the product is exact; rint rounds half to even
    order = np.argsort(i, kind="stable")
    i, q = i[order], q[order]
    starts = np.flatnonzero(np.concatenate([[True], i[1:] != i[:-1]]))
    assert len(starts) == len(p)  # every finite point is its own neighbour
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    cols = (lambda: np.ones(len(i), np.int64), lambda: qx, lambda: qy, lambda: qz, lambda: qx * qx, lambda: qx * qy, lambda: qx * qz,
            lambda: qy * qy, lambda: qy * qz, lambda: qz * qz)
    for k, col in enumerate(cols):  # (one column at a time: r = 1 holds millions of pairs)
        out[fin, k] = np.add.reduceat(col(), starts)
    return out


def covariance(mom: np.ndarray) -> np.ndarray:
    """GN5: (n, 3, 3) float64 from the moments; rows with n = 0 are zeros."""
    mom = np.asarray(mom, np.int64)
    cnt = mom[:, 0].astype(np.float64)
    safe = np.where(cnt > 0, cnt, 1.0)
    s1 = mom[:, 1:4].astype(np.float64)
    s2 = mom[:, 4:10].astype(np.float64)
    C = np.zeros((len(mom), 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        v = s2[:, k] - (s1[:, a] * s1[:, b]) / safe
        C[:, a, b] = v
        C[:, b, a] = v
    C[cnt == 0] = 0.0
    return C


def normals(mom: np.ndarray) -> dict:
    """The twin: eigh of C.  dict(normal (n, 3), curvature, gap = (l1 - l0) / l2, valid)."""
    C = covariance(mom)
    w, v = np.linalg.eigh(C)
    trace = (C[:, 0, 0] + C[:, 1, 1]) + C[:, 2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        curv = np.where(trace > 0, w[:, 0] / trace, 0.0)
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
        # the normal of a neighbourhood is defined when it spans a plane: at least 3 neighbours, rank >= 2
        valid = (mom[:, 0] >= 3) & (w[:, 1] > 1e-12 * np.maximum(w[:, 2], 1e-300))
    nrm = np.where(valid[:, None], v[:, :, 0], 0.0)
    return dict(normal=nrm, curvature=np.where(valid, curv, 0.0), gap=gap, valid=valid)


def reduce_maps(width: int, height: int, index, pixel, rng, xyz_cam) -> dict:
    """GM2 / GM3 from per-contributor rows: the smallest fp32 range wins a pixel, ties go to the lowest index.
    dict(index (H, W) int32, range (H, W) float32, xyz_cam (H, W, 3) float32, pixels = occupied, crowded = pixels with two
    contributors or more, tied = pixels whose two best contributors have the same range)."""
    index = np.asarray(index, np.int64)
    pixel = np.asarray(pixel, np.int64)
    rng = np.ascontiguousarray(rng, np.float32)
    xyz_cam = np.ascontiguousarray(xyz_cam, np.float32).reshape(-1, 3)
    bits = rng.view(np.uint32).astype(np.int64)
    order = np.lexsort((index, bits, pixel))
    sp = pixel[order]
    first = np.flatnonzero(np.concatenate([[True], sp[1:] != sp[:-1]])) if len(sp) else np.zeros(0, np.int64)
    win = order[first]
    oi = np.full(width * height, -1, np.int32)
    orng = np.zeros(width * height, np.float32)
    oxyz = np.zeros((width * height, 3), np.float32)
    oi[pixel[win]] = index[win]
    orng[pixel[win]] = rng[win]
    oxyz[pixel[win]] = xyz_cam[win]
    counts = np.diff(np.concatenate([first, [len(sp)]])) if len(sp) else np.zeros(0, np.int64)
    # pixels whose two best contributors tie on range
    tied = 0
    if len(sp):
        two = first[counts >= 2]
        tied = int((bits[order[two]] == bits[order[two + 1]]).sum())
    return dict(index=oi.reshape(height, width), range=orng.reshape(height, width), xyz_cam=oxyz.reshape(height, width, 3),
                pixels=len(win), crowded=int((counts >= 2).sum()), tied=tied)


def normal_cam(w2c: np.ndarray, n_world: np.ndarray, xyz_cam: np.ndarray) -> np.ndarray:
    """GM4 in fp64: R n, flipped to face the camera; zero normals stay zero.  w2c (3, 4) (the keyframe's fp32 matrix)."""
    R = np.asarray(w2c, np.float64)[:3, :3]
    n = np.asarray(n_world, np.float64) @ R.T
    flip = (n * np.asarray(xyz_cam, np.float64)).sum(-1) > 0
    n[flip] = -n[flip]
    return n
