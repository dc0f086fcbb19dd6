"""numpy restatement of the crack widths on the map ("Crack widths on the map", CF1-CF6 and CC1-CC6), written from
the rules and not from csrc/pcp_crack_fuse.hpp: the fusion as one vector update per keyframe (a keyframe lists a point once, so
plain fancy indexing serves), CF5 in fp64, the components by brute force over all pairs with the fp32 expression and a plain
union-find in Python, the table from the labels.  Plus the clouds and scenes the CPU and GPU suites share."""
import numpy as np

import _crack_width_ref as cw_ref

CENTRE, WIDTH = 2, 64
NO_MIN, NO_KEY = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
CLAMP_Q = 2 ** 31 - 1
FIELDS = ("seen", "views", "centres", "min_q", "max_q", "best_q", "sum_q", "best_key")


# ---- CF1-CF5 ----------------------------------------------------------------------------------------------------------------
def new_state(n):
    st = {k: np.zeros(n, np.uint64 if k in ("sum_q", "best_key") else np.uint32) for k in FIELDS}
    st["min_q"][:] = NO_MIN
    st["best_key"][:] = NO_KEY
    return st


def quantum(width):
    """CF3: rint(width * 2^20), ties to even (the product is exact in fp64 too), 2^31 - 1 from 2048 on"""
    width = np.asarray(width, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        q = np.where(width >= 2048.0, float(CLAMP_Q), np.rint(width * 1048576.0))
    return q.astype(np.uint64)


def add_frame(st, index, pixel, rng, frame, flags, width):
    """one keyframe: index (m,) distinct points, pixel (m,) linear indices, rng (m,) float32; returns the credited count"""
    index = np.asarray(index, np.int64)
    assert len(np.unique(index)) == len(index)
    f = np.asarray(flags, np.uint8).ravel()[pixel]
    w = np.asarray(width, np.float32).ravel()[pixel]
    st["seen"][index] += 1
    ok = (f & WIDTH) != 0
    i, q = index[ok], quantum(w[ok])
    st["views"][i] += 1
    st["centres"][i] += ((f[ok] & CENTRE) != 0).astype(np.uint32)
    st["sum_q"][i] += q
    st["min_q"][i] = np.minimum(st["min_q"][i], q.astype(np.uint32))
    st["max_q"][i] = np.maximum(st["max_q"][i], q.astype(np.uint32))
    key = (np.asarray(rng, np.float32)[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(frame)
    better = key < st["best_key"][i]
    st["best_key"][i[better]] = key[better]
    st["best_q"][i[better]] = q[better].astype(np.uint32)
    return int(ok.sum())


def fused_w(st):
    """CF5: floor((2 sum + views) / (2 views)) in Python integers, 0 without a view"""
    return np.array([(2 * int(s) + int(v)) // (2 * int(v)) if v else 0 for s, v in zip(st["sum_q"], st["views"])], np.int64)


def results(st):
    v = st["views"].astype(np.float64)
    has = st["views"] > 0
    safe = np.where(has, v, 1.0)
    mean = np.where(has, (st["sum_q"].astype(np.float64) / safe) * 2.0 ** -20, 0.0).astype(np.float32)
    best = np.where(has, st["best_q"].astype(np.float64) * 2.0 ** -20, 0.0).astype(np.float32)
    frame = np.where(has, (st["best_key"] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return dict(width_mean=mean, width_best=best, best_frame=frame)


# ---- CC1-CC4 ----------------------------------------------------------------------------------------------------------------
def threshold_of(radius):
    """the largest float t with (double)t <= (double)r * (double)r"""
    r2 = float(np.float32(radius)) ** 2
    t = np.float32(r2)
    if float(t) > r2:
        t = np.nextafter(t, np.float32(0))
    return np.float32(t)


def crack_points(xyz, views, min_views):
    xyz = np.asarray(xyz, np.float32)
    return (np.asarray(views).astype(np.int64) >= min_views) & np.isfinite(xyz).all(axis=1)


def links(xyz, views, min_views, radius):
    """(k, 2) int64: the linked pairs i < j of crack points, every operation of the test in fp32"""
    xyz = np.asarray(xyz, np.float32)
    who = np.flatnonzero(crack_points(xyz, views, min_views))
    p = xyz[who]
    t = threshold_of(radius)
    out = []
    for a in range(len(who) - 1):
        d = p[a + 1:] - p[a]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == np.float32
        b = np.flatnonzero(d2 <= t)
        if len(b):
            out.append(np.stack([np.full(len(b), who[a]), who[a + 1 + b]], axis=1))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 2), np.int64)


def components(xyz, views, min_views, radius, pairs=None):
    """labels (n,) int32: the lowest index of the component, -1 for a point that is no crack point"""
    n = len(xyz)
    if pairs is None:
        pairs = links(xyz, views, min_views, radius)
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for i, j in pairs.tolist():
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    label = np.full(n, -1, np.int32)
    for i in np.flatnonzero(crack_points(xyz, views, min_views)).tolist():
        label[i] = find(i)
    return label


def table(label, st, xyz):
    """ids (C,), stats (C, 5) int64: points sum_w min_w max_w centre_points, box (C, 6) float32"""
    xyz = np.asarray(xyz, np.float32)
    ids = np.unique(label[label >= 0]).astype(np.int32)
    w = fused_w(st)
    stats = np.zeros((len(ids), 5), np.int64)
    box = np.zeros((len(ids), 6), np.float32)
    for r, c in enumerate(ids.tolist()):
        mem = np.flatnonzero(label == c)
        stats[r] = (len(mem), w[mem].sum(), w[mem].min(), w[mem].max(), int((st["centres"][mem] > 0).sum()))
        box[r, :3], box[r, 3:] = xyz[mem].min(axis=0), xyz[mem].max(axis=0)
    return ids, stats, box


def check_labels(label, xyz, views, min_views, radius):
    """label against the restatement, and against scipy's components of the restatement's adjacency: the same partition, and
    every label the lowest index of its members"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    n = len(xyz)
    pairs = links(xyz, views, min_views, radius)
    want = components(xyz, views, min_views, radius, pairs)
    assert label.dtype == np.int32 and np.array_equal(label, want)
    is_cp = crack_points(xyz, views, min_views)
    assert np.array_equal(label >= 0, is_cp)
    adj = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(adj, directed=False)
    who = np.flatnonzero(is_cp)
    if len(who):
        # the same partition: label and comp determine each other on the crack points
        assert len(np.unique(np.stack([label[who], comp[who]], axis=1), axis=0)) == len(np.unique(label[who])) == len(np.unique(comp[who]))
        lowest = np.full(n, n, np.int64)
        np.minimum.at(lowest, comp[who], who)
        assert np.array_equal(label[who], lowest[comp[who]])
    return want


# ---- the clouds of the component cases --------------------------------------------------------------------------------------
def chain(n, radius, order):
    """a straight chain spaced 0.9 r along x; place p of the chain is point order[p]"""
    xyz = np.zeros((n, 3), np.float32)
    xyz[np.asarray(order), 0] = (0.9 * radius * np.arange(n)).astype(np.float32)
    return xyz


def touching_chains(radius, apart):
    """Two chains of 40 points that run away from each other; their heads are d = (a, g, 0) apart with the fp32 squared distance
    EXACTLY t (apart = False: they join) or the next float above t (apart = True: they do not).  (a, g) is searched."""
    t = threshold_of(radius)
    target = np.nextafter(t, np.float32(1)) if apart else t
    g0 = np.float32(np.sqrt(float(t)) * 0.8)
    found = None
    for step in range(200000):
        g = np.float32(g0 + np.float32(step) * np.spacing(g0))
        a = np.float32(np.sqrt(max(float(target) - float(g) * float(g), 0.0)))
        for a_try in (a, np.nextafter(a, np.float32(0)), np.nextafter(a, np.float32(1))):
            if np.float32(np.float32(a_try * a_try) + np.float32(g * g)) == target:
                found = (a_try, g)
                break
        if found:
            break
    assert found is not None, "no offset with the wanted squared distance"
    a, g = found
    k = np.arange(40, dtype=np.float32)
    step_y = np.float32(0.9 * radius)
    first = np.stack([np.zeros(40, np.float32), -k * step_y, np.zeros(40, np.float32)], axis=1)
    second = np.stack([np.full(40, a, np.float32), g + k * step_y, np.zeros(40, np.float32)], axis=1)
    xyz = np.concatenate([first, second]).astype(np.float32)
    d = xyz[40] - xyz[0]
    assert np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) == target
    return xyz


def ring(n, radius):
    rad = 0.8 * radius / (2.0 * np.sin(np.pi / n))
    ang = 2.0 * np.pi * np.arange(n) / n
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(n)], axis=1).astype(np.float32)


UNIFORM_SEED = 2


def uniform_cloud(radius, n=5000, seed=UNIFORM_SEED, degree=2.45):
    """n uniform points in a cube sized for a mean of `degree` neighbours within the radius: just below the percolation threshold
    of spheres (~2.74), where large clusters and many small ones coexist"""
    side = (n * (4.0 / 3.0) * np.pi * radius ** 3 / degree) ** (1.0 / 3.0)
    return np.random.default_rng(seed).uniform(0.0, side, (n, 3)).astype(np.float32)


def component_cases(radius=0.005):
    """name -> (xyz (n, 3) float32, views (n,) uint32, min_views).  The radius is the smallest the library takes, so that the
    long chain (18 m) fits a scene a camera sees."""
    rng = np.random.default_rng(17)
    ones = lambda n: np.ones(n, np.uint32)  # noqa: E731
    cases = {}
    n = 4100
    cases["chain_shuffled"] = (chain(n, radius, rng.permutation(n)), ones(n), 1)
    cases["chain_descending"] = (chain(n, radius, np.arange(n)[::-1]), ones(n), 1)
    cases["chains_touch"] = (touching_chains(radius, apart=False), ones(80), 1)
    cases["chains_apart"] = (touching_chains(radius, apart=True), ones(80), 1)
    base = uniform_cloud(radius, 120, seed=5, degree=2.0)
    cases["duplicates"] = (np.concatenate([base, base[::3], base[::5]]).astype(np.float32), ones(120 + 40 + 24), 1)
    cases["ring"] = (ring(300, radius), ones(300), 1)
    cases["one_cell"] = (rng.uniform(0.0, 0.9 * radius, (300, 3)).astype(np.float32), ones(300), 1)
    bad = uniform_cloud(radius, 400, seed=6, degree=4.0)
    bad[::7, 0] = np.nan
    bad[3::11, 2] = np.inf
    bad[5::13, 1] = -np.inf
    cases["non_finite"] = (bad, ones(400), 1)
    some = uniform_cloud(radius, 600, seed=7, degree=5.0)
    views = rng.integers(0, 5, 600).astype(np.uint32)
    cases["min_views_1"] = (some, views, 1)
    cases["min_views_3"] = (some, views, 3)
    cases["single"] = (np.array([[1.0, 2.0, 3.0]], np.float32), ones(1), 1)
    cases["no_crack_point"] = (some[:50], np.zeros(50, np.uint32), 1)
    cases["uniform"] = (uniform_cloud(radius), ones(5000), 1)
    return cases


# ---- the scenes of the GPU suite --------------------------------------------------------------------------------------------
def quaternion_y(deg):
    """(qw, qx, qy, qz) of a rotation about the camera's y axis"""
    h = np.radians(deg) / 2.0
    return [np.cos(h), 0.0, np.sin(h), 0.0]


def fuse_poses():
    """6 keyframes around the identity: small translations and a tilt, so that a map point lands on different pixels"""
    return np.array([[0.00, 0.00, 0.00] + quaternion_y(0.0), [0.03, 0.00, 0.00] + quaternion_y(0.0), [-0.02, 0.02, 0.05] + quaternion_y(1.5),
                     [0.00, -0.03, -0.04] + quaternion_y(-2.0), [0.05, 0.01, 0.02] + quaternion_y(3.0), [0.00, 0.00, 0.00] + quaternion_y(-1.0)])


def stripe_scene(shape=(270, 480), w0=0.05, seed=9, density=0.6):
    """A planar wall z = 3 (world) with a stripe |x - 0.1| < w0 / 2 on it, seen by 6 poses at different ranges and incidences.
    dict(cam, poses, cloud (n, 3) float32, w0, x0)."""
    h, w = shape
    cam = cw_ref.camera(shape)
    rng = np.random.default_rng(seed)
    n = int(density * h * w * 4)
    cloud = np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(-2.0, 2.0, n), np.full(n, 3.0)], axis=1).astype(np.float32)
    poses = np.array([[0.0, 0.0, 0.0] + quaternion_y(0.0), [0.0, 0.0, 0.5] + quaternion_y(0.0), [0.0, 0.0, -0.6] + quaternion_y(0.0),
                      [-0.8, 0.0, 0.0] + quaternion_y(15.0), [0.9, 0.1, 0.2] + quaternion_y(-18.0), [0.3, -0.1, -0.3] + quaternion_y(-6.0)])
    return dict(cam=cam, poses=poses, cloud=cloud, w0=w0, x0=0.1, shape=shape)


def stripe_mask(scene, c2w):
    """The stripe as keyframe c2w (3 x 4) sees it: every pixel's undistorted ray through its centre, intersected with the wall."""
    h, w = scene["shape"]
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    x, y, ok = cw_ref.rays(scene["cam"], np.stack([2 * px.ravel(), 2 * py.ravel()], axis=1))
    m = np.asarray(c2w, np.float64).reshape(3, 4)
    d = np.stack([x, y, np.ones_like(x)], axis=1) @ m[:, :3].T
    o = m[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (3.0 - o[2]) / d[:, 2]
        xw = o[0] + s * d[:, 0]
    fg = ok & (s > 0) & (np.abs(xw - scene["x0"]) < scene["w0"] / 2.0)
    return np.where(fg, 255, 0).astype(np.uint8).reshape(h, w)
