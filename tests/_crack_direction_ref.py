"""Restatement of the crack directions on the map ("Crack directions on the map", CD1-CD5), written from the rules
and not from csrc/pcp_crack_direction.hpp: the links of _crack_fuse_ref.links (brute force, the exact fp32 test), the moments
as int64 sums of the quantised offsets (exact: every sum stays far below 2^63, asserted), numpy.linalg.eigh of the fp64
covariance built by GN5's three operations, the row sums in Python integers split as CD4 says.  Plus the five clouds of known
direction the CPU and GPU suites share, and the comparison both make."""
import numpy as np

import _crack_fuse_ref as ref

QUANTA = np.float32(2.0 ** 20)
STRICT = ("chain_shuffled", "chain_descending", "chains_touch", "chains_apart", "line", "ypsilon", "helix", "arc")  # no exemptions
LINE_DIR = np.array([1.0, 2.0, 2.0]) / 3.0
HELIX_AXIS = np.array([0.0, 0.0, 1.0])
HELIX_RADIUS = 0.5


def oriented(v):
    """CD3's sign rule on the rows of v: the component of largest magnitude positive, ties to the lowest axis"""
    v = np.array(v, np.float64).reshape(-1, 3)
    b = np.argmax(np.abs(v), axis=1)  # (the first of equal maxima)
    s = np.where(v[np.arange(len(v)), b] < 0.0, -1.0, 1.0)
    return v * s[:, None]


def largest_pair(C6):
    """(l1, l2, trace, unit vector of l1) of the symmetric matrices xx xy xz yy yz zz (k, 6) by numpy.linalg.eigh"""
    C6 = np.asarray(C6, np.float64).reshape(-1, 6)
    A = np.empty((len(C6), 3, 3))
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = C6[:, 0], C6[:, 1], C6[:, 2]
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = C6[:, 1], C6[:, 3], C6[:, 4]
    A[:, 2, 0], A[:, 2, 1], A[:, 2, 2] = C6[:, 2], C6[:, 4], C6[:, 5]
    w, v = np.linalg.eigh(A)
    return w[:, 2], w[:, 1], (C6[:, 0] + C6[:, 3]) + C6[:, 5], v[:, :, 2]


def split(v):
    """CD4 on a Python integer: (lo, hi) with v = hi * 2^32 + lo, 0 <= lo < 2^32"""
    return v & 0xFFFFFFFF, v >> 32


def axis_of_rows(rows):
    """CD5 by eigh: rows (C, 20) of Python-exact integers -> link_count, axis (C, 3), axis_anisotropy, gap"""
    rows = np.asarray(rows, np.int64).reshape(-1, 20)
    c = len(rows)
    val = np.array([[float(int(r[2 * k + 1]) * 2 ** 32 + int(r[2 * k])) for k in range(10)] for r in rows], np.float64).reshape(c, 10)
    L = val[:, 0]
    axis, an, gap = np.zeros((c, 3)), np.zeros(c), np.ones(c)
    ok = L >= 2
    if ok.any():
        l1, l2, tr, v = largest_pair(val[ok, 4:] / L[ok, None])
        good = l1 > 0
        sel = np.flatnonzero(ok)[good]
        axis[sel] = oriented(v[good])
        an[sel] = l1[good] / tr[good]
        gap[sel] = (l1[good] - l2[good]) / l1[good]
    return dict(link_count=L, axis=axis, axis_anisotropy=an, axis_gap=gap)


def directions(xyz, views, min_views, radius):
    """dict(links (n,) int32, moments (n, 10) int64, valid (n,) bool, tangent (n, 3) and anisotropy (n,) float64, gap (n,), the
    relative eigen-gap (l1 - l2) / l1 (1 where invalid), label, ids (C,) int32, rows (C, 20) int64 and the axes of axis_of_rows)"""
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    pairs = ref.links(xyz, views, min_views, radius)
    label = ref.components(xyz, views, min_views, radius, pairs)
    i = np.concatenate([pairs[:, 0], pairs[:, 1]])
    j = np.concatenate([pairs[:, 1], pairs[:, 0]])
    d = xyz[j] - xyz[i]
    assert d.dtype == np.float32
    q = np.rint(d * QUANTA).astype(np.int64)  # (the product is exact: a power of two; rint: ties to even)
    assert np.abs(q).max(initial=0) <= 2 ** 20 + 1
    mom = np.zeros((n, 10), np.int64)
    np.add.at(mom[:, 0], i, 1)
    for a in range(3):
        np.add.at(mom[:, 1 + a], i, q[:, a])
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        np.add.at(mom[:, 4 + k], i, q[:, a] * q[:, b])
    cnt = mom[:, 0]
    assert cnt.max(initial=0) < 2 ** 22
    tangent, an, gap, valid = np.zeros((n, 3)), np.zeros(n), np.ones(n), np.zeros(n, bool)
    who = np.flatnonzero(cnt >= 2)
    if len(who):
        nn = cnt[who].astype(np.float64)
        s1 = mom[who, 1:4].astype(np.float64)
        s2 = mom[who, 4:].astype(np.float64)
        C = np.empty((len(who), 6))
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            C[:, k] = s2[:, k] - (s1[:, a] * s1[:, b]) / nn  # GN5: three operations
        l1, l2, tr, v = largest_pair(C)
        good = l1 > 0
        sel = who[good]
        valid[sel] = True
        tangent[sel] = oriented(v[good])
        an[sel] = l1[good] / tr[good]
        gap[sel] = (l1[good] - l2[good]) / l1[good]
    ids = np.unique(label[label >= 0]).astype(np.int32)
    row_of = {int(c): r for r, c in enumerate(ids.tolist())}
    sums = [[[0, 0] for _ in range(10)] for _ in ids]
    for p in np.flatnonzero(label >= 0).tolist():
        acc = sums[row_of[int(label[p])]]
        for k, v_ in enumerate(mom[p].tolist()):
            lo, hi = split(v_)
            acc[k][0] += lo
            acc[k][1] += hi
    assert all(0 <= w[0] < 2 ** 63 and -2 ** 63 <= w[1] < 2 ** 63 for r in sums for w in r)
    rows = np.array([[h for w in r for h in w] for r in sums], np.int64).reshape(len(ids), 20)
    out = dict(links=cnt.astype(np.int32), moments=mom, valid=valid, tangent=tangent, anisotropy=an, gap=gap, label=label, ids=ids,
               rows=rows)
    out.update(axis_of_rows(rows))
    return out


# ---- the comparison both suites make -----------------------------------------------------------------------------------------
def assert_integers(got, want, what="", moments=True):
    """links, moments, validity, ids and rows by exact equality; S1 of every row exactly zero; invalid points hold zeros"""
    assert got["links"].dtype == np.int32 and np.array_equal(got["links"], want["links"]), (what, "links")
    if moments:
        assert got["moments"].dtype == np.int64 and np.array_equal(got["moments"], want["moments"]), (what, "moments")
    assert got["ids"].dtype == np.int32 and np.array_equal(got["ids"], want["ids"]), (what, "ids")
    assert got["rows"].dtype == np.int64 and got["rows"].shape == want["rows"].shape and np.array_equal(got["rows"], want["rows"]), (what, "rows")
    # CD4: every link is counted from both ends with opposite offsets -- the value hi * 2^32 + lo of every S1 sum is exactly zero
    s1 = got["rows"][:, 2:8].astype(object)
    assert not (s1[:, 1::2] * 2 ** 32 + s1[:, 0::2]).any(), (what, "S1 sums")
    valid = got["tangent"].any(axis=1)
    assert np.array_equal(valid, want["valid"]), (what, "validity", np.flatnonzero(valid != want["valid"])[:10])
    assert not got["anisotropy"][~valid].any(), (what, "anisotropy of invalid points")
    assert np.array_equal(got["link_count"], want["link_count"]), (what, "link_count")


def _close(got_v, got_a, want_v, want_a, what):
    n = np.asarray(got_v, np.float64)
    t = want_v * np.where((n * want_v).sum(axis=1) < 0.0, -1.0, 1.0)[:, None]  # compared up to sign
    err = np.abs(n - t).max(initial=0.0)
    a, at = np.asarray(got_a, np.float64), want_a
    aerr = np.abs(a - at)
    print(what, "vectors", len(n), "largest component error", float(err), "largest anisotropy error", float(aerr.max(initial=0.0)))
    assert err <= 1e-4, (what, float(err))
    assert ((aerr <= 1e-4 * np.abs(at)) | (aerr <= 1e-9)).all(), what
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max(initial=0.0) <= 1e-6, what


def assert_vectors(got, want, name, what=""):
    """tangents and axes against eigh up to sign, with the bar of test_geometry_gpu.py::test_normals_against_eigh; points and
    cracks with a relative eigen-gap below 1e-3 are exempt: none on the STRICT cases, elsewhere at most 1 % of the points (a
    crack may have no axis to speak of: a closed ring)"""
    exempt = want["valid"] & (want["gap"] < 1e-3)
    ax_valid = want["axis"].any(axis=1)
    ax_exempt = ax_valid & (want["axis_gap"] < 1e-3)
    print(what, name, "exempt points", int(exempt.sum()), "of", int(want["valid"].sum()), "exempt axes", int(ax_exempt.sum()), "of",
          int(ax_valid.sum()))
    if name in STRICT:
        assert int(exempt.sum()) == 0 and int(ax_exempt.sum()) == 0  # the restatement alone exempts none on these
    else:
        assert exempt.sum() <= 0.01 * len(exempt)
    check = want["valid"] & ~exempt
    _close(got["tangent"][check], got["anisotropy"][check], want["tangent"][check], want["anisotropy"][check], f"{what} {name} tangents:")
    assert np.array_equal(got["axis"].any(axis=1), ax_valid), (what, name, "axis validity")
    check = ax_valid & ~ax_exempt
    _close(got["axis"][check], got["axis_anisotropy"][check], want["axis"][check], want["axis_anisotropy"][check], f"{what} {name} axes:")
    # the sign rule itself, where the largest component is clear of a tie
    for v in (np.asarray(got["tangent"], np.float64)[want["valid"]], got["axis"][ax_valid]):
        m = np.sort(np.abs(v), axis=1)
        clear = m[:, 2] - m[:, 1] > 1e-3
        assert (v[clear][np.arange(int(clear.sum())), np.argmax(np.abs(v[clear]), axis=1)] > 0).all(), (what, name, "sign rule")


def angle_deg(v, w):
    """the angle between the lines along v (k, 3) and w (3,), 0..90"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    c = np.abs(v @ np.asarray(w, np.float64)) / (np.linalg.norm(v, axis=1) * np.linalg.norm(w))
    return np.degrees(np.arccos(np.clip(c, 0.0, 1.0)))


# ---- clouds of known direction (radius 0.005) --------------------------------------------------------------------------------
def line(seed=1):
    """200 points along (1, 2, 2) / 3, spacing 1 mm, jitter 0.02 mm.  (With 0.2 mm the restatement itself is 3.3 degrees off at
    the ends of the line, whose five links all point one way, and 1.6 degrees with 0.1 mm; with 0.02 mm it is 0.32 degrees.)"""
    rng = np.random.default_rng(seed)
    s = 0.001 * np.arange(200)
    return (s[:, None] * LINE_DIR[None, :] + rng.uniform(-0.00002, 0.00002, (200, 3))).astype(np.float32)


def ypsilon_arms():
    ang = np.radians([90.0, 210.0, 330.0])
    return np.stack([np.cos(ang), np.sin(ang), np.zeros(3)], axis=1)


def ypsilon(seed=2):
    """three arms of 100 points at 120 degrees in the plane z = 0.25, spacing 1 mm from 1 mm on, jitter 0.1 mm in the plane;
    point 100 a + k is place k of arm a"""
    rng = np.random.default_rng(seed)
    s = 0.001 * (1 + np.arange(100))
    pts = np.concatenate([s[:, None] * arm[None, :] for arm in ypsilon_arms()])
    pts[:, :2] += rng.uniform(-0.0001, 0.0001, (300, 2))
    pts[:, 2] = 0.25
    return pts.astype(np.float32)


def helix(seed=3):
    """400 points on a cylinder of radius 0.5 m about z, climbing at 45 degrees to its axis, 1.5 mm apart along the curve, jitter
    0.1 mm"""
    rng = np.random.default_rng(seed)
    s = 0.0015 * np.arange(400)  # arc length
    phi = s * np.sqrt(0.5) / HELIX_RADIUS
    pts = np.stack([HELIX_RADIUS * np.cos(phi), HELIX_RADIUS * np.sin(phi), s * np.sqrt(0.5)], axis=1)
    return (pts + rng.uniform(-0.0001, 0.0001, (400, 3))).astype(np.float32)


def two_links():
    """points with exactly 0, 1 and 2 links at radius 0.005: a lone point (0), a pair (1, 1), a bent triple (1, 2, 1) with
    legs of 4.5 and 3 mm and a triangle (2, 2, 2)"""
    return np.array([[0.0, 0.0, 0.0],
                     [0.1, 0.0, 0.0], [0.104, 0.0, 0.0],
                     [0.2, 0.0, 0.0], [0.2045, 0.0, 0.0], [0.2045, 0.003, 0.0],
                     [0.3, 0.0, 0.0], [0.303, 0.0, 0.0], [0.3, 0.0, 0.003]], np.float32)


TWO_LINKS_COUNTS = [0, 1, 1, 1, 2, 1, 2, 2, 2]


def lonely_pair():
    """two duplicates only"""
    return np.array([[0.5, 0.25, 0.125], [0.5, 0.25, 0.125]], np.float32)


def direction_cases():
    """name -> (xyz, views, min_views), as _crack_fuse_ref.component_cases"""
    ones = lambda n: np.ones(n, np.uint32)  # noqa: E731
    return {"line": (line(), ones(200), 1), "ypsilon": (ypsilon(), ones(300), 1), "helix": (helix(), ones(400), 1),
            "two_links": (two_links(), ones(9), 1), "lonely_pair": (lonely_pair(), ones(2), 1)}


def check_known(name, res, k=None):
    """the known answers of the five clouds on a result (the restatement's or the library's); k: the case's own points come
    first in the cloud (a wall may follow)"""
    valid = np.asarray(res["tangent"]).any(axis=1)
    tangent = np.asarray(res["tangent"], np.float64)
    own = np.flatnonzero(res["ids"] < (k if k is not None else len(tangent)))
    if name == "line":
        assert len(own) == 1 and valid[:200].sum() >= 198
        assert angle_deg(tangent[:200][valid[:200]], LINE_DIR).max() <= 0.5
        assert (np.asarray(res["anisotropy"])[:200][valid[:200]] > 0.99).all()
        assert angle_deg(res["axis"][own], LINE_DIR).max() <= 0.5 and res["axis_anisotropy"][own[0]] > 0.99
    elif name == "ypsilon":
        assert len(own) == 1
        for a, arm in enumerate(ypsilon_arms()):
            inner = np.arange(100 * a + 10, 100 * a + 95)  # away from the junction (5 mm) and from the tip
            assert valid[inner].all() and angle_deg(tangent[inner], arm).max() <= 2.0, a
    elif name == "helix":
        assert len(own) == 1
        assert abs(float(angle_deg(res["axis"][own], HELIX_AXIS)[0]) - 45.0) <= 2.0
    elif name == "two_links":
        links = np.asarray(res["links"])[:9]
        assert links.tolist() == TWO_LINKS_COUNTS
        assert np.array_equal(valid[:9], links >= 2)
        assert not tangent[:9][links < 2].any() and not np.asarray(res["anisotropy"])[:9][links < 2].any()
    elif name == "lonely_pair":
        assert np.asarray(res["links"])[:2].tolist() == [1, 1] and not valid[:2].any() and not np.asarray(res["anisotropy"])[:2].any()
        assert len(own) == 1 and res["link_count"][own[0]] == 2 and not res["axis"][own[0]].any() and res["axis_anisotropy"][own[0]] == 0
