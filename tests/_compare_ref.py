"""numpy restatement of the map comparison ("Map comparison", MC1-MC6) and the builders of the test cases.

Offsets, the sphere test and the orientation are float32 numpy operations, each rounded on its own; the cylinder tests and the
sums are int64 arrays (Python ints in products_fit, where the bounds themselves are checked); the finish is Python floats, which
are IEEE doubles, one operation at a time."""
import math

import numpy as np

F = np.float32
Q = 2.0 ** 20
NQ = 2.0 ** 11
SUM_COLS = ("nA", "s1A", "s2aA", "s2bA", "nB", "s1B", "s2aB", "s2bB")


def threshold(r) -> np.float32:
    """The largest float t with (double)t <= (double)r * (double)r."""
    r2 = float(F(r)) * float(F(r))
    t = F(r2)
    if float(t) > r2:
        t = np.nextafter(t, F(0.0))
    return t


def search_radius(rc, L) -> np.float32:
    s = F(math.sqrt(float(F(rc)) * float(F(rc)) + float(F(L)) * float(F(L))))
    return np.nextafter(s, F(np.inf))


def squares(rc, L):
    """(rc2, L2) as Python ints: floor((fl32(x) * 2^20)^2), computed in fp64."""
    a, b = float(F(rc)) * Q, float(F(L)) * Q
    return int(math.floor(a * a)), int(math.floor(b * b))


def params_ok(rc, L, reg_error=0.0, min_points=5, orient_mode=0) -> bool:
    rc, L, reg_error = F(rc), F(L), F(reg_error)
    if not (rc >= F(0.005)) or not (L >= F(0.005)):
        return False
    if not (search_radius(rc, L) <= F(0.5)):
        return False
    return bool(reg_error >= 0 and np.isfinite(reg_error) and min_points >= 2 and 0 <= orient_mode <= 2)


def directions(xyz, normals, orient_mode=0, orient=(0, 0, 0)):
    """MC1 / MC2: (core (n,) bool, N (n, 3) int64 -- zeros where not core)."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    nrm = np.array(normals, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(xyz).all(axis=1) & np.isfinite(nrm).all(axis=1) & (np.abs(nrm) <= F(1.0)).all(axis=1) & (nrm != 0).any(axis=1)
        if orient_mode != 0:
            o = np.asarray(orient, F).reshape(1, 3)
            v = (o - xyz).astype(F) if orient_mode == 1 else np.broadcast_to(o, xyz.shape)
            dot = (nrm[:, 0] * v[:, 0] + nrm[:, 1] * v[:, 1]).astype(F) + (nrm[:, 2] * v[:, 2]).astype(F)
            nrm = np.where((dot < 0)[:, None], -nrm, nrm)
        nrm = np.where(ok[:, None], nrm, F(0))
        N = np.rint(nrm * F(NQ)).astype(np.int64)
    core = ok & ((N * N).sum(axis=1) != 0)
    N[~core] = 0
    return core, N


def _finish(s, N2, min_points, reg_error):
    nA, s1A, s2aA, s2bA, nB, s1B, s2aB, s2bB = (int(v) for v in s)
    if nB < min_points:
        return 0.0, 0.0, 1
    if nA < min_points:
        return 0.0, 0.0, 2
    scale = math.sqrt(float(N2)) * 1048576.0
    distance = (float(s1A) / float(nA) - float(s1B) / float(nB)) / scale

    def var(n, s1, s2a, s2b):
        S2 = float(s2a) + 4294967296.0 * float(s2b)
        v = (S2 - (float(s1) * float(s1)) / float(n)) / (float(n) - 1.0)
        return v if v > 0.0 else 0.0

    lod = 1.96 * math.sqrt(var(nA, s1A, s2aA, s2bA) / float(nA) + var(nB, s1B, s2aB, s2bB) / float(nB)) / scale + float(F(reg_error))
    status = (4 if distance > 0.0 else 5) if abs(distance) > lod else 3
    return distance, lod, status


class _Window:
    """The finite rows of a cloud sorted by x: a superset of the rows within r of a point (the exact tests come after)."""

    def __init__(self, pts):
        pts = np.asarray(pts, F).reshape(-1, 3)
        keep = np.flatnonzero(np.isfinite(pts).all(axis=1))
        order = keep[np.argsort(pts[keep, 0], kind="stable")]
        self.pts = pts[order]
        self.x = self.pts[:, 0].astype(np.float64)

    def near(self, p, r):
        pad = r * 1.01 + 1e-6
        a, b = np.searchsorted(self.x, [float(p[0]) - pad, float(p[0]) + pad])
        return self.pts[a:b]


def epoch_sums(p, N, cand, t, rc2, L2):
    """MC3 / MC4 for one query against candidate rows `cand`: (n, S1, S2a, S2b) as Python ints."""
    d = (cand - p[None, :]).astype(F)
    d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
    d = d[d2 <= t]
    q = np.rint(d * F(Q)).astype(np.int64)
    h = q @ N
    Q2 = (q * q).sum(axis=1)
    N2 = int(N @ N)
    hh = h * h
    inside = (hh <= L2 * N2) & (Q2 * N2 - hh <= rc2 * N2)
    h, hh = h[inside], hh[inside]
    return int(inside.sum()), int(h.sum()), int((hh & 0xFFFFFFFF).sum()), int((hh >> 32).sum())


def compare(xyz, normals, base_xyz, radius=0.03, half_length=0.05, reg_error=0.0, min_points=5, orient_mode=0, orient=(0, 0, 0)):
    """dict(distance, lod float32, status uint8, sums (n, 8) int64, direction (n, 3) int32, stats (8,) int64)."""
    assert params_ok(radius, half_length, reg_error, min_points, orient_mode)
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    s = search_radius(radius, half_length)
    t = threshold(s)
    rc2, L2 = squares(radius, half_length)
    core, N = directions(xyz, normals, orient_mode, orient)
    wa, wb = _Window(xyz), _Window(base_xyz)
    out = dict(distance=np.zeros(n, F), lod=np.zeros(n, F), status=np.zeros(n, np.uint8), sums=np.zeros((n, 8), np.int64),
               direction=N.astype(np.int32))
    for i in np.flatnonzero(core):
        p = xyz[i]
        sums = epoch_sums(p, N[i], wa.near(p, float(s)), t, rc2, L2) + epoch_sums(p, N[i], wb.near(p, float(s)), t, rc2, L2)
        out["sums"][i] = sums
        d, l, st = _finish(sums, int(N[i] @ N[i]), min_points, reg_error)
        out["distance"][i], out["lod"][i], out["status"][i] = F(d), F(l), st
    out["stats"] = stats_of(out["status"], out["sums"])
    return out


def stats_of(status, sums) -> np.ndarray:
    st = np.asarray(status)
    most = int(max(sums[:, 0].max(), sums[:, 4].max())) if len(st) else 0
    return np.array([(st != 0).sum(), (st >= 3).sum(), (st == 4).sum(), (st == 5).sum(), (st == 1).sum(), (st == 2).sum(), most, 0], np.int64)


def products_fit(xyz, normals, base_xyz, radius, half_length, orient_mode=0, orient=(0, 0, 0)) -> dict:
    """The largest products of MC3 over every offset that passes the sphere test, in Python ints (no word size)."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    s = search_radius(radius, half_length)
    t = threshold(s)
    rc2, L2 = squares(radius, half_length)
    core, N = directions(xyz, normals, orient_mode, orient)
    both = np.concatenate([xyz, np.asarray(base_xyz, F).reshape(-1, 3)])
    both = both[np.isfinite(both).all(axis=1)]
    worst = dict(h=0, hh=0, Q2N2=0, rc2N2=0, L2N2=0, neg=0)
    for i in np.flatnonzero(core):
        d = (both - xyz[i][None, :]).astype(F)
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
        q = np.rint(d[d2 <= t] * F(Q)).astype(np.int64)
        Ni = [int(v) for v in N[i]]
        N2 = sum(v * v for v in Ni)
        worst["rc2N2"] = max(worst["rc2N2"], rc2 * N2)
        worst["L2N2"] = max(worst["L2N2"], L2 * N2)
        for row in q.tolist():
            h = sum(a * b for a, b in zip(row, Ni))
            Q2 = sum(a * a for a in row)
            worst["h"] = max(worst["h"], abs(h))
            worst["hh"] = max(worst["hh"], h * h)
            worst["Q2N2"] = max(worst["Q2N2"], Q2 * N2)
            worst["neg"] = min(worst["neg"], Q2 * N2 - h * h)
    return worst


# ---- case builders: dict(xyz, normals, base, kw) with kw the keywords of compare / capi.compare_host / Context.compare ----------
TILT = 0.3
ORIGIN = np.array([3.0, -2.0, 1.0])
E_U = np.array([1.0, 0.0, 0.0])
E_V = np.array([0.0, math.cos(TILT), math.sin(TILT)])
E_N = np.array([0.0, -math.sin(TILT), math.cos(TILT)])


def _wall_points(rng, n, side, step_radius=0.0, step=0.0, sigma=0.001):
    uv = rng.uniform(0.0, side, (n, 2))
    w = rng.normal(0.0, sigma, n)
    if step_radius > 0:
        w = w + np.where(np.hypot(uv[:, 0] - side / 2, uv[:, 1] - side / 2) < step_radius, step, 0.0)
    pts = ORIGIN[None, :] + uv[:, :1] * E_U[None, :] + uv[:, 1:] * E_V[None, :] + w[:, None] * E_N[None, :]
    return pts.astype(F), uv


def eigh_normals(xyz, radius=0.05) -> np.ndarray:
    """The eigenvector of the smallest eigenvalue of the covariance of the neighbours within `radius` (numpy eigh, fp64), as
    float32; (0, 0, 0) for a point with fewer than three neighbours."""
    xyz = np.asarray(xyz, F)
    win = _Window(xyz)
    out = np.zeros((len(xyz), 3), F)
    for i, p in enumerate(xyz):
        if not np.isfinite(p).all():
            continue
        c = win.near(p, radius).astype(np.float64)
        c = c[((c - p.astype(np.float64)) ** 2).sum(axis=1) <= radius * radius]
        if len(c) >= 3:
            _, vec = np.linalg.eigh(np.cov(c.T))
            out[i] = vec[:, 0].astype(F)
    return out


def viewer(side=1.0, distance=2.0) -> np.ndarray:
    return (ORIGIN + side / 2 * E_U + side / 2 * E_V + distance * E_N).astype(F)


def wall(n=1500, seed=11, step=0.005):
    """A smaller bump: the same density on a square of side sqrt(n / 6000), the step inside a disc of a fifth of the side."""
    rng = np.random.default_rng(seed)
    side = math.sqrt(n / 6000.0)
    xyz, uv = _wall_points(rng, n, side, 0.2 * side, step)
    base, _ = _wall_points(rng, n, side)
    return dict(xyz=xyz, normals=eigh_normals(xyz), base=base, uv=uv, side=side,
                kw=dict(radius=0.03, half_length=0.05, orient_mode=1, orient=tuple(float(v) for v in viewer(side))))


def bump(seed=7):
    c = wall(6000, seed)
    assert abs(c["side"] - 1.0) < 1e-12
    return c


def boundary():
    """One query (row 0 of the map) at small multiples of 2^-20 with the normal (0, 0, 1); base rows on both sides of the axial
    bound for L = 0.05 and of the radial bound rc2 = 32765^2 = (3^2 + 4^2) * 6553^2.  Returns the case and, per base row, whether
    the rule takes it."""
    u = 2.0 ** -20
    p = np.array([3, 5, 7], np.float64) * u
    rc = 32765 * u
    offs = [((0, 0, 52428), True), ((0, 0, 52429), False), ((0, 0, -52428), True), ((0, 0, -52429), False),
            ((19659, 26212, 0), True), ((19659, 26213, 0), False), ((-19659, -26212, 9), True), ((-19660, -26212, 0), False),
            ((32765, 0, -40000), True), ((32766, 0, 0), False)]
    base = np.array([p + np.array(o, np.float64) * u for o, _ in offs]).astype(F)
    xyz = np.array([p, p + np.array([1, 0, 0]) * 0.25]).astype(F)  # (a second map point far outside the search)
    normals = np.array([[0, 0, 1], [0, 0, 1]], F)
    return dict(xyz=xyz, normals=normals, base=base, taken=[t for _, t in offs],
                kw=dict(radius=rc, half_length=0.05, min_points=2))


def sphere_corner():
    """rc and L both whole quanta; a base row whose quantised offset is the cylinder's corner (inside) while its fp32 offset lies
    outside the sphere of MC3, and one at the corner itself (inside both)."""
    u = 2.0 ** -20
    p = np.array([3, 5, 7], np.float64) * u
    base = np.array([p + np.array([32765.4, 0, 52428.4]) * u, p + np.array([32765, 0, 52428]) * u, p + np.array([0, 7, 11]) * u]).astype(F)
    xyz = np.array([p]).astype(F)
    return dict(xyz=xyz, normals=np.array([[0, 0, 1]], F), base=base, kw=dict(radius=32765 * u, half_length=52428 * u, min_points=2))


def tilted(seed=3):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 0.3, (700, 3)).astype(F)
    base = rng.uniform(0, 0.3, (700, 3)).astype(F)
    nrm = rng.normal(size=(700, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    nrm[0] = (0.6, 0.0, 0.8)        # 0.6 * 2048 = 1228.8: rint 1229, truncation 1228
    nrm[1] = (-0.6, 0.8, 0.0)
    nrm[2] = (0.5 / 2048, 0.0, 1.0)  # a tie: 0.5 rounds to even, 0
    nrm[3] = (1.5 / 2048, 0.0, 1.0)  # a tie: 1.5 rounds to even, 2
    nrm[4] = (0.0002, 0.0001, 0.0)   # every component rounds to 0: N2 == 0, status 0
    return dict(xyz=xyz, normals=nrm, base=base, kw=dict(radius=0.04, half_length=0.06, min_points=3))


def min_points_case(k=5):
    """Clusters 2 m apart with (map, base) points: (k-1, k) -> 2, (k, k) -> measured, (k, k-1) -> 1, (k-1, k-1) -> 1."""
    rng = np.random.default_rng(2)
    xyz, base, want = [], [], []
    for c, (a, b, st) in enumerate(((k - 1, k, 2), (k, k, 3), (k, k - 1, 1), (k - 1, k - 1, 1))):
        centre = np.array([2.0 * c, 0.5, -0.25])
        xyz.append(centre + rng.uniform(-0.001, 0.001, (a, 3)))
        base.append(centre + rng.uniform(-0.001, 0.001, (b, 3)))
        want += [st] * a
    xyz = np.concatenate(xyz).astype(F)
    return dict(xyz=xyz, normals=np.tile(np.array([[0, 0, 1]], F), (len(xyz), 1)), base=np.concatenate(base).astype(F), want=want,
                kw=dict(min_points=k))


def non_finite(seed=5):
    c = wall(900, seed)
    xyz, base, nrm = c["xyz"].copy(), c["base"].copy(), c["normals"].copy()
    xyz[10] = (np.nan, 0, 0)
    xyz[200] = (1.0, np.inf, 2.0)
    xyz[899] = (1.0, 2.0, -np.inf)
    base[0] = (np.nan, np.nan, np.nan)
    base[450] = (3.2, -np.inf, 1.0)
    nrm[20] = 0
    nrm[21] = (np.nan, 0, 1)
    nrm[22] = (0, 1.5, 0)
    return dict(xyz=xyz, normals=nrm, base=base, bad=[10, 200, 899, 20, 21, 22], kw=c["kw"])


def duplicates(seed=9):
    c = wall(800, seed)
    xyz = np.concatenate([c["xyz"], c["xyz"][:60], c["xyz"][:20]])
    nrm = np.concatenate([c["normals"], c["normals"][:60], c["normals"][:20]])
    base = np.concatenate([c["base"], c["xyz"][100:300], c["base"][:50]])
    # far from the wall: six copies of one point in each epoch, 2 mm apart along the normal (both variances are zero)
    spot = np.array([[7.001, 3.003, -1.007]], F)
    xyz = np.concatenate([xyz, np.repeat(spot, 6, axis=0)])
    nrm = np.concatenate([nrm, np.tile(np.array([[0.6, 0.0, 0.8]], F), (6, 1))])
    base = np.concatenate([base, np.repeat(spot - F(0.002) * np.array([[0.6, 0.0, 0.8]], F), 6, axis=0)]).astype(F)
    return dict(xyz=xyz, normals=nrm, base=base, spot=slice(len(xyz) - 6, len(xyz)), kw=c["kw"])


def wide(seed=4):
    """The search radius exactly 0.5: rc = 0.3, L the largest float with search_radius(rc, L) <= 0.5; points out to the rim."""
    L = F(0.4)
    while not (search_radius(0.3, L) <= F(0.5)):
        L = np.nextafter(L, F(0))
    assert search_radius(0.3, L) == F(0.5)
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.5, 0.5, (300, 3))
    nrm = rng.normal(size=(300, 3))
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    xyz[0], nrm[0] = (0, 0, 0), (0, 0, 1)
    xyz[1], nrm[1] = (0.01, 0.01, 0.01), (1 / math.sqrt(3),) * 3
    rim = []
    n1, e1 = np.array([1.0, 1.0, 1.0]) / math.sqrt(3), np.array([1.0, -1.0, 0.0]) / math.sqrt(2)
    for e in (-3e-7, -1e-7, 0.0, 1e-7, 3e-7):  # the cylinder's corner, the axis end and the radial rim, a hair in and out
        rim += [(0.3 + e, 0.0, float(L) + e), (0.0, 0.0, float(L) + e), (0.0, 0.3 + e, 0.0), (0.0, -(0.3 + e), -(float(L) + e))]
        # ... and the same about point 1, whose normal is the diagonal
        rim += [xyz[1] + (float(L) + e) * n1 + (0.3 + e) * e1, xyz[1] - (float(L) + e) * n1, xyz[1] + (0.3 + e) * e1]
    base = np.concatenate([rng.uniform(-0.5, 0.5, (300, 3)), np.array(rim)])
    return dict(xyz=xyz.astype(F), normals=nrm.astype(F), base=base.astype(F), kw=dict(radius=0.3, half_length=float(L), min_points=4))


def crowded(seed=6):
    """70 map points inside 2 mm (one grid cell: more than one work item's 64 queries) with 600 points of each epoch within
    the search radius (more than one LDS tile of 512 records), and a sparse frame around them."""
    rng = np.random.default_rng(seed)
    centre = np.array([1.013, 2.021, 3.017])
    knot = centre + rng.uniform(-0.001, 0.001, (70, 3))
    near_a = centre + rng.uniform(-0.03, 0.03, (530, 3)) * np.array([1, 1, 0.1])
    near_b = centre + rng.uniform(-0.03, 0.03, (600, 3)) * np.array([1, 1, 0.1]) + np.array([0, 0, 0.003])
    far_a = centre + rng.uniform(-0.4, 0.4, (200, 3))
    far_b = centre + rng.uniform(-0.4, 0.4, (200, 3))
    xyz = np.concatenate([knot, near_a, far_a]).astype(F)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], F), (len(xyz), 1))
    return dict(xyz=xyz, normals=nrm, base=np.concatenate([near_b, far_b]).astype(F), kw=dict())


def permute(case, seed=1):
    rng = np.random.default_rng(seed)
    pa, pb = rng.permutation(len(case["xyz"])), rng.permutation(len(case["base"]))
    return dict(xyz=case["xyz"][pa], normals=case["normals"][pa], base=case["base"][pb], kw=case["kw"]), pa


def same_bytes(a: dict, b: dict, keys=("distance", "lod", "status", "sums", "direction", "stats")):
    """The first key whose arrays differ in dtype, shape or bytes, or None."""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None


CASES = ("bump", "boundary", "sphere_corner", "tilted", "min_points_case", "non_finite", "duplicates", "wide", "crowded")
_made = {}


def case_and_ref(name):
    """(case, the restatement's result), computed once per process, shared among the tests and left unchanged."""
    if name not in _made:
        c = globals()[name]()
        _made[name] = (c, compare(c["xyz"], c["normals"], c["base"], **c["kw"]))
    return _made[name]
