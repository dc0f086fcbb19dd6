"""The plane-fit eigen solve of csrc/pcp_eigen33.hpp away from the GPU: a plain-Python fp64 twin of smallest_eigenpair (every
operation rounded on its own, 1 / x and 1 / sqrt(x) where the device runs mls_rcp and mls_rsqrt) that also says which branch
ran, the reference (mpmath.eigsy at 50 digits on the same fp64 matrix), the seeded case table both suites run, the error
measures, and the correctly rounded reciprocals.  tests/test_eigen33_cpu.py holds the twin to the reference,
tests/test_eigen33_gpu.py the device (pcp_selftest_eigen33) to bars derived from the twin's own errors.

Everything expensive is computed once per process (functools.lru_cache) and must be left unchanged by its users."""
import functools
import math
import os
import sys

import numpy as np

DBL_MIN = sys.float_info.min
DBL_EPSILON = sys.float_info.epsilon
U = 2.0 ** -53  # unit roundoff
FLOOR = 16 * U  # the floor of every bar: two ulp of mls_rsqrt and the three products of the normalisation, with margin
MARGIN = 8.0  # device against twin: 1-2 ulp reciprocals, another libm, fused products -- a few ulp per intermediate

BRANCHES = ("roots2", "cubic", "cubic->roots2")
CLASSES = ("separated", "caller-shaped", "exact-NaN", "ill-defined")
SEPARATED, CALLER, EXACT_NAN, ILL = range(4)
CROSS_NOISE = 256 * DBL_EPSILON  # pcp_eigen33.hpp kCrossNoise
CROSS_NOISE2 = CROSS_NOISE * CROSS_NOISE
GAP = 1e-3  # relative gap (l1 - l0) / l2 from which the vector is held to a bar

# the residual and the norm are measured in extended precision: in fp64 their own rounding would be as large as they are
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the error measures need a long double of 64 bits of mantissa or more"


# ---- the twin ---------------------------------------------------------------------------------------------------------
def _roots2(b, c):
    d = b * b - 4.0 * c
    if d < 0.0:
        d = 0.0
    sd = math.sqrt(d)
    return 0.0, 0.5 * (b - sd), 0.5 * (b + sd)


def twin(m):
    """smallest_eigenpair on m = (xx, xy, xz, yy, yz, zz): (ev, (nx, ny, nz), branch).  The vector is three NaNs where the
    longest cross product has length zero (the device: infinity times zero)."""
    m = [float(v) for v in m]
    scale = max(abs(v) for v in m)
    if scale <= DBL_MIN:
        scale = 1.0
    inv_scale = 1.0 / scale
    a00, a01, a02, a11, a12, a22 = (v * inv_scale for v in m)
    c0 = a00 * a11 * a22 + 2.0 * a01 * a02 * a12 - a00 * a12 * a12 - a11 * a02 * a02 - a22 * a01 * a01
    c1 = a00 * a11 - a01 * a01 + a00 * a22 - a02 * a02 + a11 * a22 - a12 * a12
    c2 = a00 + a11 + a22
    if abs(c0) < DBL_EPSILON:
        branch = 0
        r0, r1, r2 = _roots2(c2, c1)
    else:
        branch = 1
        inv3 = 1.0 / 3.0
        sqrt3 = math.sqrt(3.0)
        c2_3 = c2 * inv3
        a_3 = (c1 - c2 * c2_3) * inv3
        if a_3 > 0.0:
            a_3 = 0.0
        half_b = 0.5 * (c0 + c2_3 * (2.0 * c2_3 * c2_3 - c1))
        q = half_b * half_b + a_3 * a_3 * a_3
        if q > 0.0:
            q = 0.0
        rho = math.sqrt(-a_3)
        theta = math.atan2(math.sqrt(-q), half_b) * inv3
        ct, st = math.cos(theta), math.sin(theta)
        r0 = c2_3 + 2.0 * rho * ct
        r1 = c2_3 - rho * (ct + sqrt3 * st)
        r2 = c2_3 - rho * (ct - sqrt3 * st)
        if r0 >= r1:
            r0, r1 = r1, r0
        if r1 >= r2:
            r1, r2 = r2, r1
            if r0 >= r1:
                r0, r1 = r1, r0
        if r0 <= 0.0:
            branch = 2
            r0, r1, r2 = _roots2(c2, c1)
    ev = r0 * scale
    s00, s11, s22 = a00 - r0, a11 - r0, a22 - r0
    k = ((a01 * a12 - a02 * s11, a02 * a01 - s00 * a12, s00 * s11 - a01 * a01),
         (a01 * s22 - a02 * a12, a02 * a02 - s00 * s22, s00 * a12 - a01 * a02),
         (s11 * s22 - a12 * a12, a12 * a02 - a01 * s22, a01 * a12 - s11 * a02))
    ln = [(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] for v in k]
    best = 0
    if ln[1] > ln[best]:
        best = 1
    if ln[2] > ln[best]:
        best = 2
    # the longest cross product against the rounding of its own terms (the header's kCrossNoise): at or below it the
    # direction is noise, not an eigenvector -- NaN, as for a length of exactly zero
    big = max(abs(s00), abs(s11), abs(s22), abs(a01), abs(a02), abs(a12))
    big = big * big
    if not ln[best] > CROSS_NOISE2 * (big * big):
        return ev, (math.nan, math.nan, math.nan), BRANCHES[branch]
    inv_len = 1.0 / math.sqrt(ln[best])
    return ev, tuple(v * inv_len for v in k[best]), BRANCHES[branch]


def twin_many(mat):
    """twin over (n, 6): ev (n,), vec (n, 3), branch (n,) as indices into BRANCHES."""
    mat = np.asarray(mat, np.float64).reshape(-1, 6)
    ev, vec, br = np.zeros(len(mat)), np.zeros((len(mat), 3)), np.zeros(len(mat), np.int8)
    for i, m in enumerate(mat.tolist()):
        ev[i], vec[i], b = twin(m)
        br[i] = BRANCHES.index(b)
    return ev, vec, br


# ---- the reference ------------------------------------------------------------------------------------------------------
def reference(mat):
    """mpmath.eigsy at 50 digits per fp64 matrix: lam (n, 3) ascending and vec (n, 3), the unit eigenvector of lam[:, 0],
    each as a pair (hi, lo) of float64 arrays whose sum carries ~32 digits."""
    import mpmath as mp

    mat = np.asarray(mat, np.float64).reshape(-1, 6)
    n = len(mat)
    lam_hi, lam_lo, vec_hi, vec_lo = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))

    def split(x):
        hi = float(x)
        return hi, float(x - mp.mpf(hi))

    with mp.workdps(50):
        for i, (xx, xy, xz, yy, yz, zz) in enumerate(mat.tolist()):
            E, Q = mp.eigsy(mp.matrix([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]))
            order = sorted(range(3), key=lambda j: E[j])
            for c, j in enumerate(order):
                lam_hi[i, c], lam_lo[i, c] = split(E[j])
            j = order[0]
            v = [Q[0, j], Q[1, j], Q[2, j]]
            ln = mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            for c in range(3):
                vec_hi[i, c], vec_lo[i, c] = split(v[c] / ln)
    return dict(lam_hi=lam_hi, lam_lo=lam_lo, vec_hi=vec_hi, vec_lo=vec_lo)


def relative_gap(ref):
    """(l1 - l0) / l2 of the reference's eigenvalues; 0 where l2 is not positive."""
    l0, l1, l2 = ref["lam_hi"].T
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(l2 > 0, (l1 - l0) / np.where(l2 > 0, l2, 1.0), 0.0)


def errors(mat, ev, vec, ref):
    """The four measures of a result (ev (n,), vec (n, 3)) on mat (n, 6) against the reference, NaN where the vector is not
    finite: vector = |s n - v0| (s the aligning sign), value = |ev - l0| / l2, residual = |A n - ev n| / l2, norm = ||n| - 1|;
    and finite (n,) bool."""
    mat = np.asarray(mat, np.float64).reshape(-1, 6)
    fin = np.isfinite(vec).all(axis=1) & np.isfinite(ev)
    n = np.where(fin[:, None], vec, 0.0)
    e = np.where(fin, ev, 0.0)
    l2 = np.maximum(np.abs(ref["lam_hi"][:, 2]), np.abs(ref["lam_hi"][:, 0]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sgn = np.where((n * ref["vec_hi"]).sum(axis=1) < 0, -1.0, 1.0)
        dv = (n * sgn[:, None] - ref["vec_hi"]) - ref["vec_lo"]
        vector = np.sqrt((dv * dv).sum(axis=1))
        value = np.abs((e - ref["lam_hi"][:, 0]) - ref["lam_lo"][:, 0]) / l2
        A = np.empty((len(mat), 3, 3), LD)
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            A[:, a, b] = A[:, b, a] = mat[:, k].astype(LD)
        nl, el = n.astype(LD), e.astype(LD)
        r = np.einsum("nab,nb->na", A, nl) - el[:, None] * nl
        residual = (np.sqrt((r * r).sum(axis=1)) / l2.astype(LD)).astype(np.float64)
        norm = np.abs(np.sqrt((nl * nl).sum(axis=1)) - LD(1)).astype(np.float64)
    out = dict(vector=vector, value=value, residual=residual, norm=norm)
    for k in out:
        out[k] = np.where(fin, out[k], np.nan)
    out["finite"] = fin
    return out


def worst(err, cls, gap):
    """Per class: the worst value, residual and norm over the finite results, and the worst vector error over those with
    gap >= GAP (0.0 where a class has none)."""
    out = {}
    for c, name in enumerate(CLASSES):
        sel = (cls == c) & err["finite"]
        row = {k: float(err[k][sel].max()) if sel.any() else 0.0 for k in ("value", "residual", "norm")}
        sel = sel & (gap >= GAP)
        row["vector"] = float(err["vector"][sel].max()) if sel.any() else 0.0
        out[name] = row
    return out


# ---- the case table -------------------------------------------------------------------------------------------------------
def _sym6(A):
    A = 0.5 * (A + A.T)
    return [A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]]


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _spectral(rng, lam):
    Q = _rotation(rng)
    return _sym6((Q * np.asarray(lam, np.float64)) @ Q.T)


def _scale(rng):
    return math.ldexp(1.0 + rng.random(), int(rng.integers(-60, 63)))  # 2^k (1 + f), k uniform in [-60, 62]


def covariance_normals(p, q):
    """The map normals' covariance (GN2-GN5) of fp32 neighbours p (K, 3) about the fp32 query q: offsets in fp32, quantised
    to 2^-20 m, integer moments, tests/_geometry_ref.covariance."""
    import _geometry_ref as gref

    d = np.asarray(p, np.float32) - np.asarray(q, np.float32)[None, :]
    k = np.rint(d.astype(np.float64) * gref.Q).astype(np.int64)
    x, y, z = k.T
    mom = np.array([[len(k), x.sum(), y.sum(), z.sum(), (x * x).sum(), (x * y).sum(), (x * z).sum(), (y * y).sum(), (y * z).sum(),
                     (z * z).sum()]], np.int64)
    C = gref.covariance(mom)[0]
    return [C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]]


def covariance_mls(p, q):
    """The MLS fit's covariance of fp32 neighbours about the fp32 query: fp64 sums of d and d d^T, then S2 - s s / K."""
    d = np.asarray(p, np.float32).astype(np.float64) - np.asarray(q, np.float32).astype(np.float64)[None, :]
    K = float(len(d))
    s = [0.0, 0.0, 0.0]
    S = [0.0] * 6
    for dx, dy, dz in d.tolist():
        s[0] += dx; s[1] += dy; s[2] += dz
        S[0] += dx * dx; S[1] += dx * dy; S[2] += dx * dz; S[3] += dy * dy; S[4] += dy * dz; S[5] += dz * dz
    mean = [v / K for v in s]
    return [S[0] - s[0] * mean[0], S[1] - s[0] * mean[1], S[2] - s[0] * mean[2], S[3] - s[1] * mean[1], S[4] - s[1] * mean[2],
            S[5] - s[2] * mean[2]]


_FORMS = (covariance_normals, covariance_mls)
OFFSETS = (1.0, 16.0, 300.0)
CLUSTER_SIZES = (3, 5, 6, 7, 30)


def _origin(rng, offset):
    return offset * np.array([1.0, -0.83, 0.41]) + rng.uniform(-0.2, 0.2, 3)


def _frame(rng):
    Q = _rotation(rng)
    return Q[:, 0], Q[:, 1], Q[:, 2]


def _cluster(rng, kind, K, offset):
    """K fp32 points within a ball of diameter 0.025 m about a point `offset` metres out."""
    o = _origin(rng, offset)
    e1, e2, e3 = _frame(rng)
    if kind == "exact plane":
        # points of a lattice on a tilted plane whose coordinates are short binary fractions: coplanar exactly, in fp32 too
        o = np.round(o * 64.0) / 64.0
        a, b = np.array([2.0 ** -9, 0.0, 2.0 ** -10]), np.array([0.0, 2.0 ** -9, -3 * 2.0 ** -11])
        ij = [(0, 0), (1, 0), (0, 1)] + [tuple(v) for v in rng.integers(-3, 4, (K - 3, 2))]
        p = np.array([o + i * a + j * b for i, j in ij])
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
        return p.astype(np.float32)
    uvw = rng.uniform(-1.0, 1.0, (K, 3))
    uvw *= 0.012 / np.maximum(1.0, np.linalg.norm(uvw, axis=1, keepdims=True))
    if kind == "plane":
        uvw[:, 2] = rng.normal(0.0, 1e-4, K)
    elif kind == "slab":
        uvw[:, 2] *= 0.05
    return (o + uvw[:, :1] * e1 + uvw[:, 1:2] * e2 + uvw[:, 2:] * e3).astype(np.float32)


def oblique_line(rng, origin, half, count=41):
    """count collinear points, rounded to fp32, on an oblique line through `origin` (no component of the direction near 0)."""
    d = rng.uniform(0.25, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
    d /= np.linalg.norm(d)
    t = np.linspace(-half, half, count)
    return (np.asarray(origin, np.float64) + t[:, None] * d).astype(np.float32), d


@functools.lru_cache(maxsize=None)
def case_table():
    """dict(mat (N, 6) float64, cls (N,) int8 indices into CLASSES, tag (N,) str): ~20 000 matrices, seeded."""
    rng = np.random.default_rng(20261021)
    mat, cls, tag = [], [], []

    def add(m, c, t):
        mat.append([float(v) for v in m])
        cls.append(c)
        tag.append(t)

    # separated: Q diag(l) Q^T over the callers' scales, m^2 ~ 2^-40 (MLS) to quanta^2 <= 2^62 (normals), with margin
    for r01 in (1e-1, 1e-3, 1e-6, 1e-9, 1e-12, 0.0):
        for r12 in (1.0, 0.5, 1e-3):
            for _ in range(700):
                l2 = _scale(rng)
                add(_spectral(rng, [r01 * r12 * l2, r12 * l2, l2]), SEPARATED, f"l0/l1={r01:g} l1/l2={r12:g}")
    # the same class at l0 / l1 = 0, l1 / l2 = 1 with the normal near (1, 1, 1): an exact tilted plane, isotropic within.  The
    # scaled l1 l2 is 9 / 4 there, so a smallest eigenvalue of an ulp, of either sign, leaves |c0| >= DBL_EPSILON, the cubic
    # runs and returns r0 <= 0: the one reliable way into cubic->roots2
    for _ in range(900):
        n = np.array([1.0, 1.0, 1.0]) + rng.uniform(-0.05, 0.05, 3)
        n /= np.linalg.norm(n)
        add(_sym6(_scale(rng) * (np.eye(3) - np.outer(n, n))), SEPARATED, "l0/l1=0 l1/l2=1, normal near (1,1,1)")
    # caller-shaped: covariances as the stages compute them, of small neighbourhoods
    for kind in ("blob", "plane", "slab", "exact plane"):
        for offset in OFFSETS:
            for K in CLUSTER_SIZES:
                for form in _FORMS:
                    for _ in range(40 if kind == "exact plane" else 30):
                        p = _cluster(rng, kind, K, offset)
                        add(form(p, p[0]), CALLER, f"{kind} K={K} at {offset:g} m, {form.__name__[11:]}")
    # exact-NaN: every cross product of two rows of A - r0 I is exactly zero, fused or not
    add([0.0] * 6, EXACT_NAN, "zero")
    for pos in (0, 3, 5):
        for k in (-1000, -300, -60, -40, -20, -1, 0, 1, 20, 40, 62, 300, 1000):
            for f in (1.0, 1.0 + 2.0 ** -52, 1.5, 1.7320508075688772, 2.0 - 2.0 ** -52):
                m = [0.0] * 6
                m[pos] = math.ldexp(f, k)
                add(m, EXACT_NAN, "one diagonal entry")
    for _ in range(60):  # scale <= DBL_MIN: the matrix is not scaled, every product of two entries underflows to zero
        m = rng.uniform(-1.0, 1.0, 6) * rng.choice([DBL_MIN, 0.5 * DBL_MIN, 2.0 ** -1060, 5e-324 * 8])
        m[int(rng.integers(0, 6))] = rng.choice([DBL_MIN, -DBL_MIN, 5e-324, 2.0 ** -1050])
        add(m, EXACT_NAN, "scale <= DBL_MIN")
    # ill-defined: NaN and any unit vector of the (numerical) null space are both right
    for _ in range(300):
        l = _scale(rng)
        add(_spectral(rng, [l, l, l]), ILL, "l I, rotated")
    for _ in range(100):
        l = _scale(rng)
        add([l, 0.0, 0.0, l, 0.0, l], ILL, "l I")
    for r12 in (0.5, 1e-3, 1e-6):
        for _ in range(200):
            l2 = _scale(rng)
            add(_spectral(rng, [r12 * l2, r12 * l2, l2]), ILL, f"needle l0=l1={r12:g} l2")
    for d in ((1.0, 1.0, 0.0), (1.0, 2.0, 3.0)):
        d = np.array(d)
        for _ in range(100):
            add(_sym6(_scale(rng) * np.outer(d, d) / (d @ d)), ILL, "rank 1 along (%g,%g,%g)" % tuple(d))
    for _ in range(600):
        d = _rotation(rng)[:, 0]
        add(_sym6(_scale(rng) * np.outer(d, d)), ILL, "rank 1, random direction")
    for offset in (0.0, 1.0, 4.0, 16.0, 100.0, 300.0):
        for half in (0.02, 0.05, 0.1, 0.25):
            for form in _FORMS:
                for _ in range(10):
                    p, _ = oblique_line(rng, _origin(rng, offset), half)
                    add(form(p, p[int(rng.integers(0, len(p)))]), ILL, f"oblique line at {offset:g} m, {form.__name__[11:]}")
    out = dict(mat=np.array(mat, np.float64), cls=np.array(cls, np.int8), tag=np.array(tag))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def table_reference():
    """The reference over the case table, its relative gaps, the twin's results and their errors: computed once per process.
    dict(ref, gap, ev, vec, branch, err, worst)."""
    t = case_table()
    ref = reference(t["mat"])
    gap = relative_gap(ref)
    ev, vec, br = twin_many(t["mat"])
    err = errors(t["mat"], ev, vec, ref)
    return dict(ref=ref, gap=gap, ev=ev, vec=vec, branch=br, err=err, worst=worst(err, t["cls"], gap))


# ---- the reciprocals ------------------------------------------------------------------------------------------------------
def reciprocal_arguments(count=1_000_000, seed=20261022):
    """2^k (1 + f), k uniform in [-1000, 1000], f uniform in [0, 1): positive; the caller negates for 1 / x."""
    rng = np.random.default_rng(seed)
    return np.ldexp(1.0 + rng.random(count), rng.integers(-1000, 1001, count).astype(np.int32))


def _rounded_by_mpmath(x, fn):
    import mpmath as mp

    with mp.workdps(50):
        return np.array([float(fn(mp.mpf(v))) for v in np.asarray(x, np.float64).tolist()])


def rcp_by_mpmath(x):
    """RN(1 / x) through mpmath at 50 digits (float() of an mpf rounds to nearest even)."""
    return _rounded_by_mpmath(x, lambda v: 1 / v)


def rsqrt_by_mpmath(x):
    import mpmath as mp

    return _rounded_by_mpmath(x, lambda v: 1 / mp.sqrt(v))


def rcp_rounded(x):
    """RN(1 / x): IEEE division is correctly rounded."""
    return 1.0 / np.asarray(x, np.float64)


def rsqrt_rounded(x):
    """RN(1 / sqrt(x)) for positive normal x: the 64-bit long double quotient decides wherever it lies clear of a midpoint
    between two doubles (its own error is below 2 of its ulps: two correctly rounded operations), mpmath the rest."""
    x = np.asarray(x, np.float64)
    y = LD(1) / np.sqrt(x.astype(LD))
    out = y.astype(np.float64)
    lo, hi = np.nextafter(out, -np.inf), np.nextafter(out, np.inf)
    # distance of y from the nearer midpoint, in long double ulps (2^-11 of a double's)
    half_dn, half_up = (out.astype(LD) + lo.astype(LD)) / 2, (out.astype(LD) + hi.astype(LD)) / 2
    near = np.minimum(np.abs(y - half_dn), np.abs(half_up - y)) / np.spacing(y)
    hard = np.flatnonzero(near <= 4)
    out[hard] = rsqrt_by_mpmath(x[hard])
    return out


def ulps(got, want):
    """|got - want| in units of want's last place (inf where got is not finite)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want) / np.spacing(np.abs(want))
    return np.where(np.isfinite(got), d, np.inf)


# ---- the document -----------------------------------------------------------------------------------------------------------
DOCUMENT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eigen33_selftest.md")


def write_block(name, text):
    """Replace what stands between `<!-- name:begin -->` and `<!-- name:end -->` in profiles/eigen33_selftest.md by `text`
    (measured values only: the suites that compute them write them, so nothing is copied by hand).  A tree that cannot be
    written keeps its document; the assertions do not depend on it."""
    begin, end = f"<!-- {name}:begin -->", f"<!-- {name}:end -->"
    try:
        with open(DOCUMENT) as f:
            doc = f.read()
        i, j = doc.index(begin) + len(begin), doc.index(end)
        new = doc[:i] + "\n" + text.rstrip("\n") + "\n" + doc[j:]
        if new != doc:
            with open(DOCUMENT, "w") as f:
                f.write(new)
    except (OSError, ValueError):
        pass


def fmt(v):
    return "0" if v == 0 else f"{v:.2e}"
