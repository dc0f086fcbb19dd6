"""Two independent things for the tests of the map registration ("Map registration").

1. A numpy restatement of RG1-RG8: fp32 / fp64 array operations one at a time, the sums in Python integers, the solve as
   explicit loops in numpy.float64.  It shares no code with csrc/pcp_register.hpp and must agree with it bit for bit.
2. A plain fp64 point-to-plane ICP that shares none of the rules (scipy's cKDTree, unquantised residuals, numpy.linalg.lstsq):
   the yardstick for accuracy, not for bits.
"""
import math

import numpy as np

F = np.float32
D = np.float64
Q = 2.0 ** 20
NQ = 2.0 ** 11
LEVER = 2.0 ** 8
MAX_LEVER = 2 ** 18
SWEEPS = 12
DEFAULT_COND_TOL = 6.2e-3
CONVERGED, ITERATION_LIMIT, TOO_FEW_PAIRS = 0, 1, 2
DEFAULTS = dict(match_radius=0.05, max_plane_distance=0.02, sample_stride=1, max_iterations=20, min_pairs=100, tolerance=1e-5,
                cond_tol=DEFAULT_COND_TOL)


class RangeError(Exception):
    pass


def params(**over) -> dict:
    p = dict(DEFAULTS)
    p.update(over)
    return p


def params_ok(p) -> bool:
    r, d = F(p["match_radius"]), F(p["max_plane_distance"])
    return bool(F(0.005) <= r <= F(0.5) and F(0) < d <= r and p["sample_stride"] >= 1 and 1 <= p["max_iterations"] <= 1000 and
                p["min_pairs"] >= 1 and 0.0 <= p["tolerance"] <= 1.0 and 0.0 < p["cond_tol"] < 1.0)


def threshold(r) -> np.float32:
    r2 = float(F(r)) * float(F(r))
    t = F(r2)
    return np.nextafter(t, F(0)) if float(t) > r2 else t


def tau2_of(d) -> int:
    q = float(F(d)) * Q
    return int(math.floor(q * q))


# ---- RG1 ---------------------------------------------------------------------------------------------------------------------
def finite_rows(a) -> np.ndarray:
    return np.isfinite(a).all(axis=1)


def pivot_of(base):
    b = base[finite_rows(base)]
    if len(b) == 0:
        return np.zeros(3, D), 1.0
    mn, mx = b.min(axis=0).astype(D), b.max(axis=0).astype(D)
    c = (mn + mx) * 0.5
    e = mx - mn
    half = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) * 0.5
    return c, float(half) if half > 0 else 1.0


def identity():
    return [D(1), D(0), D(0), D(0)], [D(0), D(0), D(0)]


def rotation_of(q):
    w, x, y, z = (D(v) for v in q)
    one, two = D(1), D(2)
    return [one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
            two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
            two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]


def is_identity(q, t) -> bool:
    return q[0] == 1 and q[1] == 0 and q[2] == 0 and q[3] == 0 and t[0] == 0 and t[1] == 0 and t[2] == 0


def current_rows(base, q, t, c) -> np.ndarray:
    """fl32(R (b0 - c) + c + t) from the original rows; the identity and the non-finite rows give the original bytes"""
    base = np.asarray(base, F)
    if is_identity(q, t):
        return base.copy()
    R = rotation_of(q)
    fin = finite_rows(base)
    with np.errstate(all="ignore"):
        d = [base[:, a].astype(D) - c[a] for a in range(3)]
        out = base.copy()
        for a in range(3):
            r = (R[3 * a] * d[0] + R[3 * a + 1] * d[1]) + R[3 * a + 2] * d[2]
            out[fin, a] = ((r + c[a]) + t[a]).astype(F)[fin]
    return out


def matrix_of(q, t, c) -> np.ndarray:
    R = rotation_of(q)
    M = np.zeros((4, 4), D)
    for a in range(3):
        for b in range(3):
            M[a, b] = R[3 * a + b]
        rc = (R[3 * a] * c[0] + R[3 * a + 1] * c[1]) + R[3 * a + 2] * c[2]
        M[a, 3] = (c[a] - rc) + t[a]
    M[3, 3] = 1.0
    return M


# ---- RG2-RG5 -----------------------------------------------------------------------------------------------------------------
def quantise_normals(normals):
    """(N int64 (n, 3), valid (n,)) by MC1 / MC2"""
    n = np.asarray(normals, F)
    with np.errstate(all="ignore"):
        ok = np.isfinite(n).all(axis=1) & (np.abs(n) <= F(1)).all(axis=1)
        N = np.where(ok[:, None], np.rint(n * F(NQ)), 0).astype(np.int64)
    return N, ok & (N != 0).any(axis=1)


def pairs(xyz, normals, rows, base, c, p):
    """The pairs of RG2-RG4 at the current rows: dict(row, partner, g (k, 6), h, N2) as int64 arrays, before and after the trim
    (key `kept`)"""
    xyz, rows = np.asarray(xyz, F), np.asarray(rows, F)
    t = threshold(p["match_radius"])
    fin_map = np.nonzero(finite_rows(xyz))[0]
    cand = np.nonzero(finite_rows(np.asarray(base, F)))[0]
    cand = cand[cand % p["sample_stride"] == 0]
    N, valid = quantise_normals(normals)
    row_l, part_l, d_l = [], [], []
    pts = xyz[fin_map]
    if len(pts) and len(cand):
        for s in range(0, len(cand), 256):
            idx = cand[s:s + 256]
            b = rows[idx]
            dx = pts[None, :, 0] - b[:, None, 0]
            dy = pts[None, :, 1] - b[:, None, 1]
            dz = pts[None, :, 2] - b[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            j = np.argmin(d2, axis=1)  # (the first of equal values: the lowest index)
            k = np.arange(len(idx))
            ok = d2[k, j] <= t
            row_l.append(idx[ok])
            part_l.append(fin_map[j[ok]])
            d_l.append(np.stack([dx[k, j], dy[k, j], dz[k, j]], axis=1)[ok])
    if not row_l:
        z = np.zeros(0, np.int64)
        return dict(row=z, partner=z, g=np.zeros((0, 6), np.int64), h=z, N2=z, kept=np.zeros(0, bool))
    row, partner, d = np.concatenate(row_l), np.concatenate(part_l), np.concatenate(d_l)
    ok = valid[partner]
    row, partner, d = row[ok], partner[ok], d[ok]
    q = np.rint(d * F(Q)).astype(np.int64)
    Nn = N[partner]
    h = (q[:, 0] * Nn[:, 0] + q[:, 1] * Nn[:, 1]) + q[:, 2] * Nn[:, 2]
    N2 = (Nn[:, 0] * Nn[:, 0] + Nn[:, 1] * Nn[:, 1]) + Nn[:, 2] * Nn[:, 2]
    u = np.rint((rows[row].astype(D) - np.asarray(c, D)[None, :]) * LEVER).astype(np.int64)
    g = np.stack([u[:, 1] * Nn[:, 2] - u[:, 2] * Nn[:, 1], u[:, 2] * Nn[:, 0] - u[:, 0] * Nn[:, 2],
                  u[:, 0] * Nn[:, 1] - u[:, 1] * Nn[:, 0], Nn[:, 0], Nn[:, 1], Nn[:, 2]], axis=1)
    tau2 = tau2_of(p["max_plane_distance"])
    kept = np.array([int(a) * int(a) <= tau2 * int(b) for a, b in zip(h, N2)], bool)
    return dict(row=row, partner=partner, g=g, h=h, N2=N2, kept=kept)


def sums_of(pr) -> list:
    """RG5: 60 Python integers from the kept pairs"""
    k = pr["kept"]
    g, h, N2 = pr["g"][k], pr["h"][k], pr["N2"][k]
    terms = [g[:, a] * g[:, b] for a in range(6) for b in range(a, 6)] + [g[:, a] * h for a in range(6)]
    terms += [h * h, N2, np.ones(len(h), np.int64)]
    out = []
    for term in terms:
        out.append(sum(int(v) & 0xffffffff for v in term))
        out.append(sum(int(v) >> 32 for v in term))
    return out


def check_levers(rows, base, c):
    fin = finite_rows(np.asarray(base, F))
    if not fin.any():
        return
    r = np.asarray(rows, F)[fin]
    for a in range(3):
        for v in (r[:, a].min(), r[:, a].max()):
            if abs(int(np.rint((D(v) - c[a]) * LEVER))) > MAX_LEVER:
                raise RangeError("lever arm")


def evaluate(xyz, normals, base, q, t, c, p) -> list:
    rows = current_rows(base, q, t, c)
    check_levers(rows, base, c)
    return sums_of(pairs(xyz, normals, rows, base, c, p))


# ---- RG6 ---------------------------------------------------------------------------------------------------------------------
def sum_of(sums, k) -> np.float64:
    return D(float(int(sums[2 * k]))) + D(4294967296.0) * D(float(int(sums[2 * k + 1])))


def rms_of(sums) -> np.float64:
    hh, nn = sum_of(sums, 27), sum_of(sums, 28)
    return np.sqrt(hh / nn) / D(1048576.0) if nn > 0 else D(0)


def solve(sums, ell, cond_tol):
    """(update [omega, dt] of 6 float64, eigenvalues (6,), dof)"""
    with np.errstate(all="ignore"):
        one = D(1)
        sr, st = one / (D(524288.0) * D(ell)), one / D(2048.0)
        s = [sr, sr, sr, st, st, st]
        A = [[D(0)] * 6 for _ in range(6)]
        V = [[one if a == b else D(0) for b in range(6)] for a in range(6)]
        k = 0
        for a in range(6):
            for b in range(a, 6):
                A[a][b] = (sum_of(sums, k) * s[a]) * s[b]
                A[b][a] = A[a][b]
                k += 1
        rhs = [(sum_of(sums, 21 + a) * s[a]) * (one / D(2147483648.0)) for a in range(6)]
        for _ in range(SWEEPS):
            for p in range(5):
                for q in range(p + 1, 6):
                    apq = A[p][q]
                    if apq == 0:
                        continue
                    theta = (A[q][q] - A[p][p]) / (D(2) * apq)
                    t = (one if theta >= 0 else -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                    c = one / np.sqrt(t * t + one)
                    sn = t * c
                    for i in range(6):
                        aip, aiq = A[i][p], A[i][q]
                        A[i][p] = c * aip - sn * aiq
                        A[i][q] = sn * aip + c * aiq
                    for i in range(6):
                        api, aqi = A[p][i], A[q][i]
                        A[p][i] = c * api - sn * aqi
                        A[q][i] = sn * api + c * aqi
                    A[p][q] = A[q][p] = D(0)
                    for i in range(6):
                        vip, viq = V[i][p], V[i][q]
                        V[i][p] = c * vip - sn * viq
                        V[i][q] = sn * vip + c * viq
        eig = [A[a][a] for a in range(6)]
        top = D(0)
        for e in eig:
            if e > top:
                top = e
        x = [D(0)] * 6
        dof = 0
        floor_ = D(cond_tol) * top
        for e in range(6):
            if not (eig[e] > 0) or not (eig[e] >= floor_):
                continue
            dof += 1
            dot = D(0)
            for b in range(6):
                dot = dot + V[b][e] * rhs[b]
            coef = dot / eig[e]
            for a in range(6):
                x[a] = x[a] + V[a][e] * coef
        update = [x[a] / D(ell) for a in range(3)] + [x[a] for a in range(3, 6)]
    return update, np.array(eig, D), dof


def compose(q, t, update):
    one = D(1)
    hx, hy, hz = update[0] * D(0.5), update[1] * D(0.5), update[2] * D(0.5)
    ln = np.sqrt(((one + hx * hx) + hy * hy) + hz * hz)
    d = [one / ln, hx / ln, hy / ln, hz / ln]
    r = [((d[0] * q[0] - d[1] * q[1]) - d[2] * q[2]) - d[3] * q[3],
         ((d[0] * q[1] + d[1] * q[0]) + d[2] * q[3]) - d[3] * q[2],
         ((d[0] * q[2] - d[1] * q[3]) + d[2] * q[0]) + d[3] * q[1],
         ((d[0] * q[3] + d[1] * q[2]) - d[2] * q[1]) + d[3] * q[0]]
    rl = np.sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3])
    Rd = rotation_of(d)
    nt = [((Rd[3 * a] * t[0] + Rd[3 * a + 1] * t[1]) + Rd[3 * a + 2] * t[2]) + update[3 + a] for a in range(3)]
    return [v / rl for v in r], nt


def sizes_of(update, ell):
    rot = np.sqrt((update[0] * update[0] + update[1] * update[1]) + update[2] * update[2]) * D(ell)
    shift = np.sqrt((update[3] * update[3] + update[4] * update[4]) + update[5] * update[5])
    return rot, shift


# ---- RG7 / RG8 ---------------------------------------------------------------------------------------------------------------
def register(xyz, normals, base, **over) -> dict:
    """The loop from the identity: dict(T, log, status, iterations, rms, dof, pairs, sums, rows, q, t, pivot, ell)"""
    p = params(**over)
    assert params_ok(p)
    base = np.asarray(base, F).reshape(-1, 3)
    c, ell = pivot_of(base)
    q, t = identity()
    log, status, sums = [], ITERATION_LIMIT, [0] * 60
    for _ in range(p["max_iterations"]):
        sums = evaluate(xyz, normals, base, q, t, c, p)
        n_pairs = sums[58]
        row = [D(n_pairs), rms_of(sums), D(0), D(0), D(0)]
        log.append(row)
        if n_pairs < p["min_pairs"]:
            status = TOO_FEW_PAIRS
            break
        update, _, dof = solve(sums, ell, p["cond_tol"])
        row[2] = D(dof)
        row[3], row[4] = sizes_of(update, ell)
        q, t = compose(q, t, update)
        if row[3] < p["tolerance"] and row[4] < p["tolerance"]:
            status = CONVERGED
            break
    log = np.array(log, D).reshape(-1, 5)
    return dict(T=matrix_of(q, t, c), log=log, status=status, iterations=len(log), rms=float(log[-1, 1]), dof=int(log[-1, 2]),
                pairs=int(log[-1, 0]), sums=np.array(sums, np.int64), rows=current_rows(base, q, t, c), q=q, t=t, pivot=c, ell=ell)


# ---- the plain ICP -------------------------------------------------------------------------------------------------------------
def rodrigues(w) -> np.ndarray:
    a = float(np.linalg.norm(w))
    if a == 0:
        return np.eye(3)
    k = np.asarray(w, D) / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def plain_icp(xyz, normals, base, match_radius=0.05, max_plane_distance=0.02, max_iterations=20, tolerance=1e-5, rcond=DEFAULT_COND_TOL, **_):
    """Point-to-plane ICP in plain fp64 with the loop's stopping rule and nothing else of the rules: dict(T (4, 4), spectrum (6,)
    descending eigenvalues of the last normal matrix, columns in metres, divided by the pairs; pairs, rms, iterations)"""
    from scipy.spatial import cKDTree

    xyz = np.asarray(xyz, D)
    nrm = np.asarray(normals, D)
    ok = np.isfinite(xyz).all(axis=1) & np.isfinite(nrm).all(axis=1) & (np.abs(nrm).sum(axis=1) > 0)
    xyz, nrm = xyz[ok], nrm[ok]
    nrm = nrm / np.linalg.norm(nrm, axis=1)[:, None]
    b0 = np.asarray(base, D)
    b0 = b0[np.isfinite(b0).all(axis=1)]
    c = (b0.min(axis=0) + b0.max(axis=0)) * 0.5
    ell = 0.5 * float(np.linalg.norm(b0.max(axis=0) - b0.min(axis=0))) or 1.0
    tree = cKDTree(xyz)
    T = np.eye(4)
    spectrum, rms, used, it = np.zeros(6), 0.0, 0, 0
    for it in range(1, max_iterations + 1):
        b = b0 @ T[:3, :3].T + T[:3, 3]
        dist, j = tree.query(b)
        m = dist <= match_radius
        r = np.einsum("ij,ij->i", xyz[j[m]] - b[m], nrm[j[m]])
        keep = np.abs(r) <= max_plane_distance
        bb, nn, r = b[m][keep], nrm[j[m]][keep], r[keep]
        used, rms = len(r), float(np.sqrt(np.mean(r * r))) if len(r) else 0.0
        J = np.hstack([np.cross(bb - c, nn) / ell, nn])
        spectrum = np.linalg.eigvalsh(J.T @ J / max(1, len(r)))[::-1]
        x = np.linalg.lstsq(J, r, rcond=math.sqrt(rcond))[0]  # (lstsq's rcond bounds singular values: the root of the eigenvalues')
        w, dt = x[:3] / ell, x[3:]
        Rd = rodrigues(w)
        S = np.eye(4)
        S[:3, :3] = Rd
        S[:3, 3] = c - Rd @ c + dt
        T = S @ T
        if np.linalg.norm(w) * ell < tolerance and np.linalg.norm(dt) < tolerance:
            break
    return dict(T=T, spectrum=spectrum, pairs=used, rms=rms, iterations=it, pivot=c, ell=ell)


def pose_error(T, T_true, pivot):
    """(translation error at the pivot in metres, rotation error in radians)"""
    T, T_true = np.asarray(T, D), np.asarray(T_true, D)
    p = np.append(np.asarray(pivot, D), 1.0)
    shift = float(np.linalg.norm((T @ p - T_true @ p)[:3]))
    R = T[:3, :3] @ T_true[:3, :3].T
    angle = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1.0) / 2.0)))
    # (acos loses the small angles: the skew part keeps them)
    skew = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return shift, float(np.linalg.norm(skew)) if angle < 1e-3 else angle


# ---- scenes ------------------------------------------------------------------------------------------------------------------
ORIGIN = np.array([3.0, -2.0, 1.0])


def planted(shift_mm=4.0, angle_deg=0.2, about=(0.5, 0.5, 0.5)) -> np.ndarray:
    """The planted motion that takes the base onto the map: a rotation about an oblique axis through ORIGIN + about, then a
    shift, of the given sizes"""
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    R = rodrigues(axis * math.radians(angle_deg))
    d = np.array([0.6, 0.64, -0.48]) * shift_mm * 1e-3
    p = ORIGIN + np.asarray(about, D)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = p - R @ p + d
    return T


def moved(points, T) -> np.ndarray:
    p = np.asarray(points, D)
    return (p @ T[:3, :3].T + T[:3, 3]).astype(F)


def _walls(rng, per_wall, which, sigma):
    pts, nrm = [], []
    for axis in which:
        uv = rng.uniform(0.0, 1.0, (per_wall, 2))
        w = rng.normal(0.0, sigma, per_wall)
        p = np.zeros((per_wall, 3))
        p[:, axis] = w
        p[:, (axis + 1) % 3] = uv[:, 0]
        p[:, (axis + 2) % 3] = uv[:, 1]
        n = np.zeros((per_wall, 3))
        n[:, axis] = 1.0
        pts.append(p + ORIGIN[None, :])
        nrm.append(n)
    return np.concatenate(pts).astype(F), np.concatenate(nrm).astype(F)


def corner(seed=21, per_wall=2000, resampled=False, walls=(0, 1, 2), sigma=0.001):
    """Three orthogonal 1 m walls (or some of them), analytic normals.  The base is the map moved by the inverse of the planted
    motion: an exact rigid copy, or (resampled) a new sample from the next seed with its own noise."""
    xyz, normals = _walls(np.random.default_rng(seed), per_wall, walls, sigma)
    src = _walls(np.random.default_rng(seed + 1), per_wall, walls, sigma)[0] if resampled else xyz
    T = planted()
    return dict(xyz=xyz, normals=normals, base=moved(src, np.linalg.inv(T)), T_true=T, kw={})


def wall_alone(seed=21):
    """One wall (normal +z): the motion along z and about x and y is observable, the rest is not"""
    return corner(seed, walls=(2,))


def changed(seed=7):
    """The step-in-a-disc wall of the comparison's tests (5 mm inside a disc of radius 0.2), the base moved by the inverse of a
    planted motion that a single wall can show: 4 mm along its normal and 0.2 degrees about an in-plane axis"""
    import _compare_ref as cref

    c = cref.bump(seed)
    e_n, e_u = cref.E_N, cref.E_U
    mid = cref.ORIGIN + 0.5 * cref.E_U + 0.5 * cref.E_V
    R = rodrigues(e_u * math.radians(0.2))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mid - R @ mid + 0.004 * e_n
    normals = np.tile(e_n.astype(F), (len(c["xyz"]), 1))
    return dict(xyz=c["xyz"], normals=normals, base=moved(c["base"], np.linalg.inv(T)), T_true=T, e_n=e_n, e_u=e_u, e_v=cref.E_V, kw={})


# ---- hand-built boundary cases: dict(xyz, normals, base, kw, pairs) evaluated once at the identity -----------------------------
QF = F(1.0) / F(Q)
UP = (0.0, 0.0, 1.0)
FAR = (0.25, 0.5, 0.0)  # a second base row without a partner: it gives the base's box an extent


def _case(xyz, normals, base, pairs, **kw):
    return dict(xyz=np.array(xyz, F).reshape(-1, 3), normals=np.array(normals, F).reshape(-1, 3), base=np.array(base, F).reshape(-1, 3),
                pairs=pairs, kw=kw)


def _offset_with_d2(target) -> tuple:
    """(dx, dy) with fl32(dx * dx + dy * dy) == target, dx near the root and dy a small multiple of 2^-20"""
    root = F(math.sqrt(float(target)))
    dx = np.array([root + F(k) * np.spacing(root) for k in range(-40, 1)], F)[:, None]
    dy = (np.arange(0, 4096, dtype=F) * QF)[None, :]
    hit = np.argwhere((dx * dx + dy * dy) == target)
    assert len(hit), "no offset lands on the threshold"
    return F(dx[hit[0][0], 0]), F(dy[0, hit[0][1]])


def boundaries() -> dict:
    r = 0.05
    t = threshold(r)
    at, beyond = _offset_with_d2(t), _offset_with_d2(np.nextafter(t, F(1)))
    cases = dict(
        d2_at_the_threshold=_case([(at[0], at[1], 0)], [UP], [(0, 0, 0), FAR], 1, match_radius=r, max_plane_distance=r),
        d2_one_ulp_beyond=_case([(beyond[0], beyond[1], 0)], [UP], [(0, 0, 0), FAR], 0, match_radius=r, max_plane_distance=r),
        trim_on_the_boundary=_case([(100 * QF, 0, 2000 * QF), (0.25, 0, -2000 * QF)], [UP, UP], [(0, 0, 0), (0.25, 0, 0)], 2,
                                   max_plane_distance=float(2000 * QF)),
        trim_one_quantum_beyond=_case([(100 * QF, 0, 2001 * QF), (0.25, 0, -2001 * QF)], [UP, UP], [(0, 0, 0), (0.25, 0, 0)], 0,
                                      max_plane_distance=float(2000 * QF)),
        tie_goes_to_the_lowest_index=_case([(0.01, 0, 0), (0, 0.01, 0), (0, 0, 0.01)], [(0, 0, 1), (0, 1, 0), (1, 0, 0)], [(0, 0, 0), FAR], 1),
        tie_the_other_way=_case([(0, 0.01, 0), (0.01, 0, 0)], [(0, 1, 0), (0, 0, 1)], [(0, 0, 0), FAR], 1),
        duplicated_map_point=_case([(0.01, 0.002, 0.001)] * 2, [(0.6, 0, 0.8), (0, 1, 0)], [(0, 0, 0), FAR], 1),
        invalid_nearest_normal=_case([(0.01, 0, 0), (0.02, 0, 0), (0.25, 0.51, 0), (0.25, 0.52, 0)],
                                     [(0, 0, 0), UP, (float("nan"), 0, 1), UP], [(0, 0, 0), FAR], 0),
        nothing_in_reach=_case([(0.0501, 0, 0), (0.3, 0.5, 0)], [UP, UP], [(0, 0, 0), FAR], 0),
        non_finite_base_rows=_case([(0.01, 0, 0.001), (0.25, 0.49, -0.001)], [UP, UP],
                                   [(float("nan"), 0, 0), (0, 0, 0), (0, float("inf"), 0), FAR, (0, 0, float("-inf"))], 2),
        lever_at_the_limit=_case([(1024.0, 0.01, 0.001)], [UP], [(-1024.0, 0, 0), (1024.0, 0, 0)], 1),
    )
    return cases


def lever_beyond() -> dict:
    """|u| = 2^18 + 1: the rows lie 1024.00390625 m (exact in fp32) either side of the pivot 0"""
    return _case([(1024.0, 0.01, 0.001)], [UP], [(-1024.00390625, 0, 0), (1024.00390625, 0, 0)], None)


def strided(seed=5, n=700, n_base=100) -> dict:
    """A small wall; the base has 100 = 3 * 33 + 1 rows, every third is a query"""
    rng = np.random.default_rng(seed)
    xyz, normals = _walls(rng, n, (2,), 0.001)
    xyz = (xyz - ORIGIN.astype(F) * F(1)).astype(F) * F(0.3)
    base = (xyz[rng.permutation(n)[:n_base]] + rng.normal(0, 0.002, (n_base, 3))).astype(F)
    return dict(xyz=xyz, normals=normals, base=base, pairs=None, kw=dict(sample_stride=3))


def hand_sums(rank: int, seed=3, big=False) -> tuple:
    """(60 Python integers, ell): pairs on three walls (rank 6), one wall (rank 3) or none (rank 0) with a planted residual;
    big: every term multiplied so that the sums pass 2^63 (only the halves hold them)"""
    rng = np.random.default_rng(seed)
    total = [0] * 30
    axes = {6: (0, 1, 2), 3: (2,), 0: ()}[rank]
    for axis in axes:
        for _ in range(40):
            N = [0, 0, 0]
            N[axis] = 2048
            u = [int(v) for v in rng.integers(-200, 201, 3)]
            u[axis] = 0
            h = int(rng.integers(-3000, 3001)) * 2048
            g = [u[1] * N[2] - u[2] * N[1], u[2] * N[0] - u[0] * N[2], u[0] * N[1] - u[1] * N[0]] + N
            terms = [g[a] * g[b] for a in range(6) for b in range(a, 6)] + [g[a] * h for a in range(6)] + [h * h, 2048 * 2048, 1]
            total = [a + b for a, b in zip(total, terms)]
    if big:
        total = [v * 2 ** 34 + (12345 if v else 0) for v in total]
        assert rank == 0 or abs(total[0]) > 2 ** 63
    out = []
    for v in total:
        out += [v & 0xffffffff, v >> 32]
    return out, 0.8


# ---- shapes at which the search kernel itself can go wrong: tight clusters far apart, each inside one cell of the grid ---------
def grid_cells(xyz, base, radius):
    """The cell (ix, iy, iz) of every finite map point and every finite base row in the grid a registration call builds over
    both clouds: build_radius_grid's edge and grid_coords' fp32 sequence restated.  (cells of the map, cells of the base,
    the edge)"""
    xyz, base = np.asarray(xyz, F), np.asarray(base, F)
    both = np.concatenate([xyz[finite_rows(xyz)], base[finite_rows(base)]])
    mn, mx = both.min(axis=0), both.max(axis=0)
    ext = [max(float(F(mx[a] - mn[a])), 1e-3) for a in range(3)]
    by_density = F(np.cbrt(ext[0] * ext[1] * ext[2] / (8.0 * len(both))))
    cell = max(F(radius) * F(1.001), by_density)
    inv = F(1.0) / cell
    count = [int(np.floor(F(mx[a] - mn[a]) * inv)) + 1 for a in range(3)]

    def cells(p):
        c = np.floor((p - mn[None, :]) * inv).astype(np.int64)
        return np.minimum(np.maximum(c, 0), np.array(count)[None, :] - 1)

    return cells(xyz), cells(base), float(cell)


SHAPE_PLAN = ((70, 10), (0, 30), (20, 0), (5, 600), (64, 20), (3, 64), (130, 1))  # (base rows, map points) per cluster


def shapes(seed=17) -> dict:
    """dict(xyz, normals, base, kw, map_cluster, base_cluster): clusters 0.425 m apart on a 2 x 2 x 2 lattice (8.49 cells of
    0.05005: no cluster near a cell's face), 0.2 mm wide.  A: 70 base rows and 10 map points (two work items, the second short);
    B: map points only; C: base rows only; D: 600 map points and 5 base rows in ONE cell (its neighbour row crosses the
    512-record tile); E: exactly 64 base rows and 20 map points (the item's last lane is the cell's last base record); F: 64 map
    points and 3 base rows; G: 130 base rows and 1 map point (three items on one partner).  shape_occupancy checks that the
    grid puts every cluster into one cell of its own."""
    rng = np.random.default_rng(seed)
    xyz, base, mc, bc = [], [], [], []
    for k, (nb, nm) in enumerate(SHAPE_PLAN):
        centre = np.array([0.425 * (k % 2), 0.425 * ((k // 2) % 2), 0.425 * (k // 4)]) + 0.123
        xyz.append(centre + rng.uniform(-1e-4, 1e-4, (nm, 3)))
        base.append(centre + rng.uniform(-1e-4, 1e-4, (nb, 3)))
        mc += [k] * nm
        bc += [k] * nb
    xyz, base = np.concatenate(xyz).astype(F), np.concatenate(base).astype(F)
    n = rng.normal(size=(len(xyz), 3))
    normals = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F)
    perm = rng.permutation(len(base))
    return dict(xyz=xyz, normals=normals, base=base[perm], kw=dict(max_plane_distance=0.05), pairs=70 + 5 + 64 + 3 + 130,
                map_cluster=np.array(mc), base_cluster=np.array(bc)[perm])


def shape_occupancy(c, radius=0.05) -> list:
    """Per cluster of shapes(): (base rows, map points) of the ONE cell that holds all of it, by the grid's own formula;
    raises when a cluster spans two cells, shares its cell, or has a neighbour within reach"""
    cm, cb, _ = grid_cells(c["xyz"], c["base"], radius)
    out, seen = [], []
    for k in range(len(SHAPE_PLAN)):
        mine = np.concatenate([cm[c["map_cluster"] == k], cb[c["base_cluster"] == k]])
        cell = tuple(mine[0])
        assert (mine == mine[0]).all(), f"cluster {k} spans more than one cell"
        assert all(max(abs(a - b) for a, b in zip(cell, other)) > 2 for other in seen), f"cluster {k} has another within reach"
        seen.append(cell)
        out.append((int((cb == mine[0]).all(axis=1).sum()), int((cm == mine[0]).all(axis=1).sum())))
    return out


def one_cell_base(seed=19) -> dict:
    """The whole base is one row repeated 100 times (one cell whatever the grid), beside a small wall"""
    rng = np.random.default_rng(seed)
    xyz, normals = _walls(rng, 400, (2,), 0.001)
    xyz = ((xyz - ORIGIN.astype(F)) * F(0.2)).astype(F)
    base = np.tile(np.array([[0.1, 0.1, 0.002]], F), (100, 1))
    return dict(xyz=xyz, normals=normals, base=base, kw={}, pairs=100)
