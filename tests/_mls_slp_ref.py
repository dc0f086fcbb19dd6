"""Numpy restatement of MovingLeastSquares' SAMPLE_LOCAL_PLANE upsampling [upstream]: the fp32
sample table loop of computeMLSPointNormal, and projectPointSimpleToPolynomialSurface on top of the numpy twin's
per-point MLSResult (oracle.np_oracle.mls_results)."""
import numpy as np

f32, f64 = np.float32, np.float64


def table(radius: float, step: float):
    """(u, v) float32 arrays in emission order:
        for (float u = -(float)R; u <= R; u += (float)S)
          for (float v = -(float)R; v <= R; v += (float)S)
            if (u * u + v * v < R * R) emit(u, v)
    with fp32 squares and sum (no fusion), both comparisons in double."""
    r, d = f32(radius), f32(step)
    rr = f64(radius) * f64(radius)
    us, vs = [], []
    u = -r
    while f64(u) <= radius:
        v = -r
        while f64(v) <= radius:
            s = f32(u * u) + f32(v * v)
            if f64(s) < rr:
                us.append(u)
                vs.append(v)
            v = f32(v + d)
        u = f32(u + d)
    return np.array(us, f32), np.array(vs, f32)


def _oriented(res, flip: bool):
    """The MLSResult with its plane normal negated: v = n.unitOrthogonal() negates with it, u = n x v stays; the fitted
    polynomial in the flipped frame is z'(u, v') = -z(u, -v'), so the coefficients of (1, v, v^2, u, uv, u^2) become
    (-c0, c1, -c2, -c3, c4, -c5) -- negations only, exact."""
    if not flip:
        return res
    r = dict(res)
    r["normal"] = -res["normal"]
    r["v"] = -res["v"]
    c = np.array(res["c_vec"], f64)
    if len(c) == 6:
        c = c * np.array([-1.0, 1.0, -1.0, -1.0, 1.0, -1.0])
    r["c_vec"] = c
    return r


def emit(results, radius: float, step: float, order: int, flips=None):
    """Rows of every fitted point (results[i] not None) in ascending index, the table's samples in order:
    dict(xyz (m, 3) float32, normal (m, 3) float32, curvature (m,) float32, index (m,) int32).  flips[i]: orient point i's
    plane the other way (the sign the fit under test chose)."""
    tu, tv = table(radius, step)
    T = len(tu)
    xyz, nrm, curv, idx = [], [], [], []
    for i, res in enumerate(results):
        if res is None:
            continue
        r = _oriented(res, bool(flips[i]) if flips is not None else False)
        n, ua, va, mean = (np.asarray(r[k], f64) for k in ("normal", "u", "v", "mean"))
        c = np.asarray(r["c_vec"], f64)
        u = tu.astype(f64)
        v = tv.astype(f64)
        w = np.zeros(T)
        normal = np.tile(n, (T, 1))
        if order > 1 and r["fitted"] and np.isfinite(c[0]):
            # getPolynomialPartialDerivative, order 2: monomials (ui, vi) = (0,0) (0,1) (0,2) (1,0) (1,1) (2,0)
            w = c[0] + v * c[1] + v * v * c[2] + u * c[3] + u * v * c[4] + u * u * c[5]
            zu = c[3] + v * c[4] + 2.0 * u * c[5]
            zv = c[1] + 2.0 * v * c[2] + u * c[4]
            normal = n[None, :] - (zu[:, None] * ua[None, :] + zv[:, None] * va[None, :])
            ln = np.sqrt((normal * normal).sum(axis=1))
            normal = normal / np.where(ln > 0, ln, 1.0)[:, None]
        p = mean[None, :] + u[:, None] * ua[None, :] + v[:, None] * va[None, :] + w[:, None] * n[None, :]
        xyz.append(p.astype(f32))
        nrm.append(normal.astype(f32))
        curv.append(np.full(T, r["curvature"], f32))
        idx.append(np.full(T, i, np.int32))
    if not xyz:
        z3 = np.zeros((0, 3), f32)
        return dict(xyz=z3, normal=z3.copy(), curvature=np.zeros(0, f32), index=np.zeros(0, np.int32))
    return dict(xyz=np.concatenate(xyz), normal=np.concatenate(nrm), curvature=np.concatenate(curv),
                index=np.concatenate(idx))
