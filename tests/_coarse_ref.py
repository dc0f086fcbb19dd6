"""A numpy restatement of the coarse registration ("Coarse registration", CG1-CG8) and the scenes of its tests: fp32 /
fp64 operations one at a time, counts and sums in Python integers, the Jacobi as explicit loops in numpy.float64.  It shares no
code with csrc/pcp_coarse.hpp and must agree with it bit for bit.  The helpers of RG1 / MC1 come from _register_ref.py, which is
a restatement of its own."""
import math

import numpy as np

import _register_ref as rref
from _register_ref import D, F, Q, finite_rows, quantise_normals, threshold

M64 = (1 << 64) - 1
NO_KEY = M64
FOUND, TOO_FEW_INLIERS = 0, 2
ACCEPTED, REPEAT, SHORT_SIDE, SIDE_MISMATCH, THIN = range(5)
SWEEPS = 12
REFIT = 65536.0
MAX_REFIT = 1 << 26
RUNNER_TRACE = 2.969615506024416
DEFAULTS = dict(support_radius=0.2, normal_radius=0.1, inlier_distance=0.05, min_side=0.3, side_tolerance=0.05, min_angle_deg=15.0,
                map_stride=4, base_stride=4, min_neighbours=20, min_offplane_permille=100, ratio_q8=230, mutual=1, hypotheses=4096,
                min_inliers=10, seed=1)


class RangeError(Exception):
    pass


def params(**over) -> dict:
    p = dict(DEFAULTS)
    p.update(over)
    return p


# ---- CG1 / CG2 -----------------------------------------------------------------------------------------------------------------
def edges2(p) -> list:
    E = int(np.rint(float(F(p["support_radius"])) * Q))
    return [((k * E) // 8) ** 2 for k in range(8)]


def descriptors(xyz, normals, stride, p) -> dict:
    """dict(desc (slots, 64) uint16, total (slots,) uint32, state (slots,) uint8) of one cloud"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    slots = (n + stride - 1) // stride
    desc, total, state = np.zeros((slots, 64), np.uint16), np.zeros(slots, np.uint32), np.zeros(slots, np.uint8)
    fin = finite_rows(xyz) if n else np.zeros(0, bool)
    N, valid = quantise_normals(normals) if n else (np.zeros((0, 3), np.int64), np.zeros(0, bool))
    pts = xyz[fin]
    t, e2 = threshold(p["support_radius"]), edges2(p)
    for s in range(slots):
        i = s * stride
        if not fin[i] or not valid[i]:
            continue
        dx, dy, dz = pts[:, 0] - xyz[i, 0], pts[:, 1] - xyz[i, 1], pts[:, 2] - xyz[i, 2]
        near = ((dx * dx + dy * dy) + dz * dz) <= t
        q = [np.rint(v[near] * F(Q)).astype(np.int64) for v in (dx, dy, dz)]
        Ni = [int(v) for v in N[i]]
        N2 = (Ni[0] * Ni[0] + Ni[1] * Ni[1]) + Ni[2] * Ni[2]
        h = (q[0] * Ni[0] + q[1] * Ni[1]) + q[2] * Ni[2]
        hh = h * h
        W = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) * N2 - hh
        assert (W >= 0).all() and N2 * e2[7] < 2 ** 62
        radial, height = np.zeros(len(h), np.int64), np.zeros(len(h), np.int64)
        for k in range(1, 8):
            radial += e2[k] * N2 <= W
            height += e2[k] * N2 <= hh
        hist = [int(v) for v in np.bincount(radial * 8 + height, minlength=64)]
        cnt = int(near.sum())
        plane = sum(hist[0::8])
        ok = cnt >= p["min_neighbours"] and (cnt - plane) * 1000 >= p["min_offplane_permille"] * cnt
        total[s] = cnt
        state[s] = 2 if ok else 1
        if ok:
            desc[s] = [c * 65535 // cnt for c in hist]
    return dict(desc=desc, total=total, state=state)


# ---- CG3 -----------------------------------------------------------------------------------------------------------------------
def best_two(dq, dc) -> np.ndarray:
    """(K, 2) uint64: the least and the second least key (L1 << 32 | ordinal) of every query over the candidates"""
    dq, dc = np.asarray(dq, np.int64).reshape(-1, 64), np.asarray(dc, np.int64).reshape(-1, 64)
    out = np.full((len(dq), 2), NO_KEY, np.uint64)
    if len(dc) == 0:
        return out
    ordinal = np.arange(len(dc), dtype=np.int64)
    for s in range(0, len(dq), 64):
        l1 = np.abs(dq[s:s + 64, None, :] - dc[None, :, :]).sum(axis=2)
        keys = np.sort((l1 << 32) | ordinal[None, :], axis=1)[:, :2].astype(np.uint64)
        out[s:s + 64, :keys.shape[1]] = keys
    return out


def correspondences(base_keys, map_keys, p) -> np.ndarray:
    pairs = []
    for b in range(len(base_keys)):
        best, second = int(base_keys[b, 0]), int(base_keys[b, 1])
        if best == NO_KEY:
            continue
        l1, m = best >> 32, best & 0xffffffff
        if second != NO_KEY and not l1 * 256 <= p["ratio_q8"] * (second >> 32):
            continue
        if p["mutual"] and (int(map_keys[m, 0]) & 0xffffffff) != b:
            continue
        pairs.append((b, m))
    return np.array(pairs, np.int32).reshape(-1, 2)


# ---- CG4 -----------------------------------------------------------------------------------------------------------------------
def draw(seed, h, slot, C) -> int:
    z = (seed + 0x9E3779B97F4A7C15 * (3 * h + slot + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z = z ^ (z >> 31)
    return ((z >> 32) * C) >> 32


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _triangle(p1, p2, p3, min_sin2):
    p1, p2, p3 = ([D(v) for v in p] for p in (p1, p2, p3))
    a = [p2[k] - p1[k] for k in range(3)]
    b = [p3[k] - p1[k] for k in range(3)]
    c = [p3[k] - p2[k] for k in range(3)]
    cen = [((p1[k] + p2[k]) + p3[k]) / D(3) for k in range(3)]
    ln = [_norm(a), _norm(b), _norm(c)]
    n = _cross(a, b)
    n2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    s = [ln[0] * ln[0], ln[1] * ln[1], ln[2] * ln[2]]
    with np.errstate(all="ignore"):
        bound = D(min_sin2) * (((s[0] * s[1]) * s[2]) / min(s[0], min(s[1], s[2])))
    if not n2 > 0 or not n2 >= bound:
        return False, ln, None, cen
    nl = np.sqrt(n2)
    e1 = [a[k] / ln[0] for k in range(3)]
    e3 = [n[k] / nl for k in range(3)]
    return True, ln, (e1, _cross(e3, e1), e3), cen


def min_sin2_of(p) -> float:
    s = math.sin(float(F(p["min_angle_deg"])) * 0.017453292519943295)
    return s * s


def identity_frame(pivot) -> np.ndarray:
    return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, *[float(v) for v in pivot], 0, 0, 0], D)


def hypothesis(cb, cm, pivot, h, p) -> dict:
    """dict(code, triple, frame (15,): R row-major, pivot, t)"""
    C = len(cb)
    t = tuple(draw(p["seed"], h, s, C) for s in range(3))
    out = dict(code=ACCEPTED, triple=t, frame=identity_frame(pivot))
    if t[0] == t[1] or t[0] == t[2] or t[1] == t[2]:
        return dict(out, code=REPEAT)
    s2 = min_sin2_of(p)
    okm, lm, em, cenm = _triangle(cm[t[0]], cm[t[1]], cm[t[2]], s2)
    okb, lb, eb, cenb = _triangle(cb[t[0]], cb[t[1]], cb[t[2]], s2)
    if any(not lm[s] >= D(float(F(p["min_side"]))) for s in range(3)):
        return dict(out, code=SHORT_SIDE)
    if any(not abs(lm[s] - lb[s]) <= D(float(F(p["side_tolerance"]))) for s in range(3)):
        return dict(out, code=SIDE_MISMATCH)
    if not okm or not okb:
        return dict(out, code=THIN)
    R = [(em[0][i] * eb[0][j] + em[1][i] * eb[1][j]) + em[2][i] * eb[2][j] for i in range(3) for j in range(3)]
    c = [D(v) for v in pivot]
    d = [cenb[a] - c[a] for a in range(3)]
    tt = [(cenm[a] - c[a]) - ((R[3 * a] * d[0] + R[3 * a + 1] * d[1]) + R[3 * a + 2] * d[2]) for a in range(3)]
    return dict(out, frame=np.array(R + c + tt, D))


# ---- CG5 -----------------------------------------------------------------------------------------------------------------------
def tau2_of(p) -> int:
    q = float(F(p["inlier_distance"])) * Q
    return int(math.floor(q * q))


def inliers(frame, cb, cm, p) -> np.ndarray:
    """(C,) bool under one frame"""
    cb, cm = np.asarray(cb, F).reshape(-1, 3), np.asarray(cm, F).reshape(-1, 3)
    R, c, t = frame[:9], frame[9:12], frame[12:15]
    with np.errstate(all="ignore"):
        d = [cb[:, a].astype(D) - c[a] for a in range(3)]
        o = [(((R[3 * a] * d[0] + R[3 * a + 1] * d[1]) + R[3 * a + 2] * d[2]) + c[a]) + t[a] for a in range(3)]
        off = [cm[:, a] - o[a].astype(F) for a in range(3)]
        small = (np.abs(off[0]) <= F(1)) & (np.abs(off[1]) <= F(1)) & (np.abs(off[2]) <= F(1))
        q = [np.where(small, np.rint(v * F(Q)), 0).astype(np.int64) for v in off]
    return small & (((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) <= tau2_of(p))


# ---- CG6 -----------------------------------------------------------------------------------------------------------------------
def refit(cb, cm, flags, pivot_b, pivot_m) -> np.ndarray:
    pb, pm = [D(v) for v in pivot_b], [D(v) for v in pivot_m]
    n, su, sv, suv = 0, [0, 0, 0], [0, 0, 0], [0] * 9
    for k in np.nonzero(flags)[0]:
        u = [int(np.rint((D(cb[k][a]) - pb[a]) * D(REFIT))) for a in range(3)]
        v = [int(np.rint((D(cm[k][a]) - pm[a]) * D(REFIT))) for a in range(3)]
        if any(abs(w) > MAX_REFIT for w in u + v):
            raise RangeError("the refit's range")
        n += 1
        for a in range(3):
            su[a] += u[a]
            sv[a] += v[a]
            for b in range(3):
                suv[3 * a + b] += u[a] * v[b]
    out = identity_frame(pivot_b)
    if n < 3:
        return out
    dn = D(float(n))
    S = [(D(float(n * suv[k] - su[k // 3] * sv[k % 3])) / dn) / D(4294967296.0) for k in range(9)]
    A = np.zeros((4, 4), D)
    A[0, 0] = (S[0] + S[4]) + S[8]
    A[0, 1], A[0, 2], A[0, 3] = S[5] - S[7], S[6] - S[2], S[1] - S[3]
    A[1, 1] = (S[0] - S[4]) - S[8]
    A[1, 2], A[1, 3] = S[1] + S[3], S[6] + S[2]
    A[2, 2] = (S[4] - S[0]) - S[8]
    A[2, 3] = S[5] + S[7]
    A[3, 3] = (S[8] - S[0]) - S[4]
    for a in range(4):
        for b in range(a):
            A[a, b] = A[b, a]
    V = np.eye(4, dtype=D)
    one, two = D(1), D(2)
    for _ in range(SWEEPS):
        for p_ in range(3):
            for q_ in range(p_ + 1, 4):
                apq = A[p_, q_]
                if apq == 0:
                    continue
                with np.errstate(over="ignore"):  # (theta * theta may overflow: t is then 0, as in the header)
                    theta = (A[q_, q_] - A[p_, p_]) / (two * apq)
                    t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                sn = t * c
                for i in range(4):
                    aip, aiq = A[i, p_], A[i, q_]
                    A[i, p_] = c * aip - sn * aiq
                    A[i, q_] = sn * aip + c * aiq
                for i in range(4):
                    api, aqi = A[p_, i], A[q_, i]
                    A[p_, i] = c * api - sn * aqi
                    A[q_, i] = sn * api + c * aqi
                A[p_, q_] = A[q_, p_] = 0
                for i in range(4):
                    vip, viq = V[i, p_], V[i, q_]
                    V[i, p_] = c * vip - sn * viq
                    V[i, q_] = sn * vip + c * viq
    top = 0
    for a in range(1, 4):
        if A[a, a] > A[top, top]:
            top = a
    q = [V[a, top] for a in range(4)]
    ln = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    if not ln > 0:
        return out
    sign = -one if q[0] < 0 else one
    q = [(v / ln) * sign for v in q]
    R = rref.rotation_of(q)
    mu = [(D(float(su[a])) / dn) / D(REFIT) for a in range(3)]
    mv = [(D(float(sv[a])) / dn) / D(REFIT) for a in range(3)]
    t = [((pm[a] - pb[a]) + mv[a]) - ((R[3 * a] * mu[0] + R[3 * a + 1] * mu[1]) + R[3 * a + 2] * mu[2]) for a in range(3)]
    return np.array(R + pb + t, D)


def matrix_of_frame(f) -> np.ndarray:
    R, c, t = f[:9], f[9:12], f[12:15]
    M = np.zeros((4, 4), D)
    for a in range(3):
        for b in range(3):
            M[a, b] = R[3 * a + b]
        rc = (R[3 * a] * c[0] + R[3 * a + 1] * c[1]) + R[3 * a + 2] * c[2]
        M[a, 3] = (c[a] - rc) + t[a]
    M[3, 3] = 1.0
    return M


def transform_of(M, c):
    """rg::from_matrix for a rigid M: (q, t) about pivot c (Shepperd's branches)"""
    R = [D(M[a, b]) for a in range(3) for b in range(3)]
    one, two, quarter = D(1), D(2), D(0.25)
    tr = (R[0] + R[4]) + R[8]
    if tr >= R[0] and tr >= R[4] and tr >= R[8]:
        s = np.sqrt(one + tr) * two
        q = [quarter * s, (R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s]
    elif R[0] >= R[4] and R[0] >= R[8]:
        s = np.sqrt(((one + R[0]) - R[4]) - R[8]) * two
        q = [(R[7] - R[5]) / s, quarter * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s]
    elif R[4] >= R[8]:
        s = np.sqrt(((one + R[4]) - R[0]) - R[8]) * two
        q = [(R[2] - R[6]) / s, (R[1] + R[3]) / s, quarter * s, (R[5] + R[7]) / s]
    else:
        s = np.sqrt(((one + R[8]) - R[0]) - R[4]) * two
        q = [(R[3] - R[1]) / s, (R[2] + R[6]) / s, (R[5] + R[7]) / s, quarter * s]
    ln = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [v / ln for v in q]
    t = [(D(M[a, 3]) - c[a]) + ((R[3 * a] * c[0] + R[3 * a + 1] * c[1]) + R[3 * a + 2] * c[2]) for a in range(3)]
    return q, t


def consensus(cb, cm, pivot_b, pivot_m, p) -> dict:
    """CG4-CG6 over the correspondences' coordinates: dict(scored, refused, winner, runner_up, refit, kept, status, winner_h, triple,
    frame (the kept one, None with status 2), inliers (C,) uint8, codes (hypotheses,))"""
    C = len(cb)
    out = dict(scored=0, refused=0, winner=0, runner_up=0, refit=0, kept=0, status=TOO_FEW_INLIERS, winner_h=-1, triple=(-1, -1, -1),
               frame=None, inliers=np.zeros(C, np.uint8), codes=[])
    if C < 3:
        return out
    hyp = [hypothesis(cb, cm, pivot_b, h, p) for h in range(p["hypotheses"])]
    out["codes"] = [h["code"] for h in hyp]
    good = [h for h, v in enumerate(hyp) if v["code"] == ACCEPTED]
    out["scored"], out["refused"] = len(good), p["hypotheses"] - len(good)
    if not good:
        return out
    counts = [int(inliers(hyp[h]["frame"], cb, cm, p).sum()) for h in good]
    win = max(range(len(good)), key=lambda k: (counts[k], -k))
    Rw = hyp[good[win]]["frame"][:9]
    for k, h in enumerate(good):
        tr = D(0)
        for a in range(9):
            tr = tr + hyp[h]["frame"][a] * Rw[a]
        if tr < RUNNER_TRACE and counts[k] > out["runner_up"]:
            out["runner_up"] = counts[k]
    out.update(winner=counts[win], winner_h=good[win], triple=hyp[good[win]]["triple"])
    if counts[win] < p["min_inliers"]:
        return out
    flags = inliers(hyp[good[win]]["frame"], cb, cm, p)
    again = refit(cb, cm, flags, pivot_b, pivot_m)
    flags2 = inliers(again, cb, cm, p)
    out.update(refit=int(flags2.sum()), frame=hyp[good[win]]["frame"], kept=counts[win], inliers=flags.astype(np.uint8), status=FOUND)
    if out["refit"] >= counts[win]:
        out.update(frame=again, kept=out["refit"], inliers=flags2.astype(np.uint8))
    return out


def register(xyz, normals, base, base_normals, **over) -> dict:
    """The whole stage: the report's entries, T (4, 4), inliers, and the stages' arrays (desc_map, desc_base, keys, pairs, cb, cm)"""
    p = params(**over)
    xyz, base = np.asarray(xyz, F).reshape(-1, 3), np.asarray(base, F).reshape(-1, 3)
    dm, db = descriptors(xyz, normals, p["map_stride"], p), descriptors(base, base_normals, p["base_stride"], p)
    vm, vb = np.nonzero(dm["state"] == 2)[0], np.nonzero(db["state"] == 2)[0]
    bk, mk = best_two(db["desc"][vb], dm["desc"][vm]), best_two(dm["desc"][vm], db["desc"][vb])
    pairs = correspondences(bk, mk, p)
    cb, cm = base[vb[pairs[:, 0]] * p["base_stride"]], xyz[vm[pairs[:, 1]] * p["map_stride"]]
    pivot_b, _ = rref.pivot_of(base)
    pivot_m, _ = rref.pivot_of(xyz)
    out = consensus(cb, cm, pivot_b, pivot_m, p)
    T = np.eye(4)
    if out["status"] == FOUND:
        q, t = transform_of(matrix_of_frame(out["frame"]), pivot_b)
        T = rref.matrix_of(q, t, pivot_b)
    out.update(keypoints_map=int((dm["state"] != 0).sum()), keypoints_base=int((db["state"] != 0).sum()), valid_map=len(vm), valid_base=len(vb),
               correspondences=len(pairs), T=T, desc_map=dm, desc_base=db, base_keys=bk, map_keys=mk, pairs=pairs, cb=cb, cm=cm,
               pivot_b=pivot_b, pivot_m=pivot_m)
    return out


REPORT = ("keypoints_map", "keypoints_base", "valid_map", "valid_base", "correspondences", "scored", "refused", "winner", "runner_up", "refit",
          "kept", "status", "winner_h", "triple")


def same_report(got, want):
    """None, or the first entry of the report that differs"""
    for k in REPORT:
        if got[k] != want[k]:
            return f"{k}: {got[k]} != {want[k]}"
    return None


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def _patch(rng, n, origin, eu, ev, sigma):
    """n points on the parallelogram origin + a eu + b ev (a, b uniform in [0, 1)), noise sigma along the normal"""
    eu, ev = np.asarray(eu, D), np.asarray(ev, D)
    nrm = np.cross(eu, ev)
    nrm /= np.linalg.norm(nrm)
    ab = rng.uniform(0.0, 1.0, (n, 2))
    return np.asarray(origin, D) + ab[:, :1] * eu + ab[:, 1:] * ev + rng.normal(0.0, sigma, n)[:, None] * nrm, np.tile(nrm, (n, 1))


# (origin, eu, ev, share of the points): walls of unequal size about a corner, a pilaster on the long wall and a step on the floor.
# The room is 2.4 m long: RG6 measures its lever arms from the base's ORIGINAL midpoint, so a shift of 3 m on a room half that
# size leaves the fine registration 4 of its 6 directions ("Coarse registration", the scene).
ROOM = (((0, 0, 0), (2.4, 0, 0), (0, 0, 1.6), 0.28), ((0, 0, 0), (0, 1.5, 0), (0, 0, 1.2), 0.14), ((0, 0, 0), (2.4, 0, 0), (0, 1.5, 0), 0.26),
        ((0.9, 0, 0), (0, 0.25, 0), (0, 0, 1.6), 0.04), ((1.3, 0, 0), (0, 0.25, 0), (0, 0, 1.6), 0.04), ((0.9, 0.25, 0), (0.4, 0, 0), (0, 0, 1.6), 0.06),
        ((1.7, 0.8, 0), (0, 0.7, 0), (0, 0, 0.3), 0.04), ((1.7, 0.8, 0.3), (0.7, 0, 0), (0, 0.7, 0), 0.08), ((1.7, 0.8, 0), (0.7, 0, 0), (0, 0, 0.3), 0.06))
# What the scene's tests pass to the coarse stage.  At 500 points per square metre a support of 0.25 m holds some 140 points, so
# the ratio test would drop most of the true matches with the false ones: the mutual test alone stays, every second row is a
# keypoint, and more triples are drawn because most hold a false match and are refused by their sides.
ROOM_KW = dict(support_radius=0.25, ratio_q8=256, map_stride=2, base_stride=2, hypotheses=16384)


def room_points(seed, n=6000, sigma=0.001):
    rng = np.random.default_rng(seed)
    pts, nrm = zip(*[_patch(rng, int(round(n * share)), o, eu, ev, sigma) for o, eu, ev, share in ROOM])
    return np.concatenate(pts) + rref.ORIGIN, np.concatenate(nrm)


def planted(angle=1.2, shift=3.0) -> np.ndarray:
    """The motion that takes the base onto the map: `angle` rad about an oblique axis through the room, then `shift` m"""
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    R = rref.rodrigues(axis * angle)
    p = rref.ORIGIN + np.array([1.0, 0.7, 0.6])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = p - R @ p + np.array([0.6, 0.64, -0.48]) * shift
    return T


def _based(xyz, normals, src, src_n, T) -> dict:
    inv = np.linalg.inv(T)
    return dict(xyz=np.asarray(xyz, F), normals=np.asarray(normals, F), base=rref.moved(src, inv),
                base_normals=(np.asarray(src_n, D) @ inv[:3, :3].T).astype(F), T_true=T)


def room(seed=31, n=6000) -> dict:
    """dict(xyz, normals, base, base_normals, T_true): the map, and a resampled noisy copy (the next seed) moved by the inverse
    of the planted motion; analytic normals, the base's turned with it"""
    xyz, normals = room_points(seed, n)
    src, src_n = room_points(seed + 1, n)
    return _based(xyz, normals, src, src_n, planted())


def box_corners(points) -> np.ndarray:
    p = np.asarray(points, D)
    p = p[np.isfinite(p).all(axis=1)]
    mn, mx = p.min(axis=0), p.max(axis=0)
    return np.array([[x, y, z] for x in (mn[0], mx[0]) for y in (mn[1], mx[1]) for z in (mn[2], mx[2])])


def corner_gap(T_a, T_b, points) -> float:
    """the farthest any corner of the points' box lands apart under the two transforms, in metres"""
    c = box_corners(points)
    a = c @ T_a[:3, :3].T + T_a[:3, 3]
    b = c @ T_b[:3, :3].T + T_b[:3, 3]
    return float(np.linalg.norm(a - b, axis=1).max())


SYMMETRIC_KW = dict(support_radius=0.25, ratio_q8=256, mutual=0, map_stride=2, base_stride=2, hypotheses=2048)


def symmetric_corner(seed=5, per_wall=1500) -> dict:
    """Three equal 1 m walls about a corner at (2, 2, 2), the second and third the first with its coordinates moved round
    (x, y, z) -> (z, x, y): the turns by 120 degrees about the diagonal map the points onto themselves exactly.  The base is
    an exact copy moved by the inverse of a planted motion."""
    rng = np.random.default_rng(seed)
    wall = np.stack([rng.normal(0.0, 0.001, per_wall), rng.uniform(0.0, 1.0, per_wall), rng.uniform(0.0, 1.0, per_wall)], axis=1).astype(F) + F(2)
    nrm = np.tile(np.array([1, 0, 0], F), (per_wall, 1))
    xyz = np.concatenate([wall, wall[:, [2, 0, 1]], wall[:, [1, 2, 0]]])
    normals = np.concatenate([nrm, nrm[:, [2, 0, 1]], nrm[:, [1, 2, 0]]])
    T = planted(angle=0.7, shift=1.0)
    return _based(xyz, normals, xyz, normals, T)


# ---- shapes at which the kernels themselves can go wrong -------------------------------------------------------------------------
CROWD_KW = dict(support_radius=0.02, min_neighbours=5, min_offplane_permille=0)
CROWD_CELL = 700


def crowded(seed=23) -> dict:
    """dict(xyz, normals, cluster): 700 points inside ONE cell of the descriptor stage's grid at support_radius 0.02 (its walk
    crosses the 512-record tile, its queries fill eleven work items), and 20 points at each corner of the 0.3 m box, the corners
    themselves among them: keypoints on the grid's faces, whose neighbouring rows are clipped.  Random unit normals."""
    rng = np.random.default_rng(seed)
    cell = float(F(0.02) * F(1.001))
    centre = 7.5 * cell
    pts, cluster = [rng.uniform(centre - 0.008, centre + 0.008, (CROWD_CELL, 3))], [0] * CROWD_CELL
    for k in range(8):
        corner = np.array([0.3 * (k & 1), 0.3 * ((k >> 1) & 1), 0.3 * (k >> 2)])
        inward = np.where(corner > 0, -1.0, 1.0)
        pts.append(np.concatenate([corner[None, :], corner + inward * rng.uniform(0.0, 0.015, (19, 3))]))
        cluster += [k + 1] * 20
    xyz = np.concatenate(pts).astype(F)
    n = rng.normal(size=(len(xyz), 3))
    perm = rng.permutation(len(xyz))
    return dict(xyz=xyz[perm], normals=(n / np.linalg.norm(n, axis=1)[:, None]).astype(F)[perm], cluster=np.array(cluster)[perm])


def crowd_occupancy(c) -> int:
    """The number of points in the cell that holds the crowd, by the grid's own formula (rref.grid_cells); raises when the crowd
    spans two cells"""
    cells, _, _ = rref.grid_cells(c["xyz"], np.zeros((0, 3), F), CROWD_KW["support_radius"])
    mine = cells[c["cluster"] == 0]
    assert (mine == mine[0]).all(), "the crowd spans more than one cell"
    return int((cells == mine[0]).all(axis=1).sum())


BLOB_KW = dict(support_radius=0.05, min_neighbours=1, min_offplane_permille=0, ratio_q8=256, mutual=0, map_stride=1, base_stride=1,
               min_side=0.01, side_tolerance=0.5, inlier_distance=0.05)


def blob(n, seed, duplicates=0) -> tuple:
    """(xyz, normals): n points in a 0.1 m cube with random unit normals, every one a keypoint with a valid descriptor under
    BLOB_KW; the last `duplicates` rows repeat the first ones (equal descriptors)"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.0, 0.1, (n, 3)).astype(F) + F(1)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)
    if duplicates:
        xyz[n - duplicates:] = xyz[:duplicates]
        nrm[n - duplicates:] = nrm[:duplicates]
    return xyz, nrm
