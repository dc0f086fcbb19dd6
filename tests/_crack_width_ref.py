"""numpy restatement of the crack width maps ("Crack width maps", CW1-CW9), written from the rules and not from
csrc/pcp_crack_width.hpp: the ridge and the traces in int64 arrays (all sites step together), the moments by gathering each
site's window and summing (q - r) directly, the plane by numpy.linalg.eigh of the same covariance, the rays and the width in
fp64.  Plus the scenes the CPU and GPU suites share."""
import numpy as np

import _mask_edt_ref as edt_ref

SITE, CENTRE, NEAR, FAR, PLANE, RAYS, WIDTH = 1, 2, 4, 8, 16, 32, 64
INTEGER_BITS = SITE | CENTRE | NEAR | FAR
Q = 65536.0  # CW4: 2^16 quanta per metre
LIMIT = np.float32(64.0)
# the reference's distortion coefficients (scripts/genNormAndDistanceMask.py :881; OpenCV order k1 k2 p1 p2 k3)
DISTORTION = dict(k1=0.003043514741045163, k2=0.06634739187544138, p1=-0.000217681797407554, p2=-0.0006654964142658197, k3=0.0)
IDENTITY_POSE = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


# ---- CW1-CW3 ------------------------------------------------------------------------------------------------------------
def integer_stage(mask, d2, nearest, threshold=0):
    """flags (bits 0-3) uint8 (H, W), edges int32 (H, W, 4), w2d2 uint32 (H, W) from the mask and ITS distance maps."""
    mask = np.asarray(mask, np.uint8)
    h, w = mask.shape
    fg = mask.astype(np.int64) > threshold
    flags = np.where(fg, SITE, 0).astype(np.uint8)
    edges = np.full((h, w, 4), -1, np.int32)
    w2d2 = np.zeros((h, w), np.uint32)
    if fg.all() or not fg.any():  # CW1: without background a site is a site and nothing else
        return flags, edges, w2d2
    # CW2: d2[p] >= d2[q] for every 8-neighbour inside the image (outside: padded with 0, below every d2)
    d = np.zeros((h + 2, w + 2), np.int64)
    d[1:-1, 1:-1] = d2
    top = np.zeros((h, w), np.int64)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                top = np.maximum(top, d[dy:dy + h, dx:dx + w])
    flags[fg & (d[1:-1, 1:-1] >= top)] |= CENTRE
    # CW3
    ys, xs = np.nonzero(fg)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    e1 = nearest[ys, xs].astype(np.int64)
    vx, vy = xs - e1 % w, ys - e1 // w
    ax, ay = np.abs(vx), np.abs(vy)
    a = np.maximum(ax, ay)
    assert (a > 0).all()
    found = {}
    for s, bit, col in ((-1, NEAR, 0), (1, FAR, 2)):
        sx, sy = s * np.sign(vx), s * np.sign(vy)
        live = np.arange(len(xs))
        fx, fy = xs.copy(), ys.copy()
        ok = np.zeros(len(xs), bool)
        ex, ey = np.full(len(xs), -1, np.int64), np.full(len(xs), -1, np.int64)
        k = 0
        while len(live):
            k += 1
            assert k <= max(w, h)
            qx = xs[live] + sx[live] * ((2 * k * ax[live] + a[live]) // (2 * a[live]))
            qy = ys[live] + sy[live] * ((2 * k * ay[live] + a[live]) // (2 * a[live]))
            inside = (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
            hit = np.zeros(len(live), bool)
            hit[inside] = ~fg[qy[inside], qx[inside]]
            at = live[hit]
            ok[at] = True
            ex[at], ey[at] = fx[at] + qx[hit], fy[at] + qy[hit]
            go = inside & ~hit
            fx[live[go]], fy[live[go]] = qx[go], qy[go]
            live = live[go]
        flags[ys[ok], xs[ok]] |= bit
        edges[ys, xs, col], edges[ys, xs, col + 1] = ex, ey
        found[s] = ok
    both = found[-1] & found[1]
    e = edges[ys[both], xs[both]].astype(np.int64)
    w2d2[ys[both], xs[both]] = ((e[:, 2] - e[:, 0]) ** 2 + (e[:, 3] - e[:, 1]) ** 2).astype(np.uint32)
    return flags, edges, w2d2


# ---- CW4-CW5 ------------------------------------------------------------------------------------------------------------
def members(index, xyz):
    """(member (H, W) bool, q (H, W, 3) int64)"""
    xyz = np.asarray(xyz, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (np.asarray(index) >= 0) & (np.abs(xyz) < LIMIT).all(axis=-1)
    q = np.zeros(xyz.shape, np.int64)
    q[ok] = np.rint(xyz[ok].astype(np.float64) * Q).astype(np.int64)  # exact product; rint rounds half to even
    return ok, q


def moments_at(member, q, ys, xs, radius):
    """(len, 13) int64 at the given pixels: n r[3] S1'[3] S2'[6], each window gathered and summed directly"""
    h, w = member.shape
    out = np.zeros((len(ys), 13), np.int64)
    for i, (y, x) in enumerate(zip(ys.tolist(), xs.tolist())):
        y0, y1, x0, x1 = max(0, y - radius), min(h, y + radius), max(0, x - radius), min(w, x + radius)
        qq = q[y0:y1, x0:x1][member[y0:y1, x0:x1]]
        n = len(qq)
        out[i, 0] = n
        if n == 0:
            continue
        r = (2 * qq.sum(axis=0) + n) // (2 * n)  # floor towards -inf
        d = qq - r
        assert np.abs(d).max() < 2 ** 23
        s2 = d.T @ d
        out[i, 1:4], out[i, 4:7] = r, d.sum(axis=0)
        out[i, 7:13] = (s2[0, 0], s2[0, 1], s2[0, 2], s2[1, 1], s2[1, 2], s2[2, 2])
    return out


# ---- CW6-CW8 in fp64 ------------------------------------------------------------------------------------------------------
def _distort(cam, x, y):
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    rc = 1.0 + cam["k1"] * r2 + cam["k2"] * r2 * r2 + cam["k3"] * r2 * r2 * r2
    t1 = 2.0 * x * y
    return rc * x + cam["p1"] * t1 + cam["p2"] * (r2 + 2.0 * x2), rc * y + cam["p1"] * (r2 + 2.0 * y2) + cam["p2"] * t1


def rays(cam, E):
    """E (k, 2) doubled edge points -> (x, y, good): ten fixed-point steps, then the redistortion within 1e-3 px"""
    E = np.asarray(E, np.float64)
    u, v = E[:, 0] / 2 + 0.5, E[:, 1] / 2 + 0.5
    x0, y0 = (u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"]
    x, y = x0.copy(), y0.copy()
    with np.errstate(all="ignore"):
        for _ in range(10):
            x2, y2 = x * x, y * y
            r2 = x2 + y2
            rc = 1.0 + cam["k1"] * r2 + cam["k2"] * r2 * r2 + cam["k3"] * r2 * r2 * r2
            t1 = 2.0 * x * y
            x, y = (x0 - (cam["p1"] * t1 + cam["p2"] * (r2 + 2.0 * x2))) / rc, (y0 - (cam["p1"] * (r2 + 2.0 * y2) + cam["p2"] * t1)) / rc
        xd, yd = _distort(cam, x, y)
        good = (np.abs(cam["fx"] * xd + cam["cx"] - u) <= 1e-3) & (np.abs(cam["fy"] * yd + cam["cy"] - v) <= 1e-3)
    return x, y, good


def float_stage(cam, mom, edges):
    """The twin of CW6-CW8 for k sites: mom (k, 13), edges (k, 4) (-1 = missing).  dict(plane_ok, normal (k, 3), offset = -n.c,
    gap = (l1 - l0) / trace, rays_ok, near / far (k, 3), width, cos = the smaller incidence |n . d| / |d| of the two rays)."""
    mom = np.asarray(mom, np.int64)
    k = len(mom)
    n = mom[:, 0].astype(np.float64)
    safe = np.where(n > 0, n, 1.0)
    s1 = mom[:, 4:7].astype(np.float64)
    C = np.zeros((k, 3, 3))
    for e, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[:, a, b] = C[:, b, a] = mom[:, 7 + e].astype(np.float64) - (s1[:, a] * s1[:, b]) / safe
    C[n == 0] = 0.0
    lam, vec = np.linalg.eigh(C)
    trace = lam.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(trace > 0, (lam[:, 1] - lam[:, 0]) / trace, 0.0)
    nrm = vec[:, :, 0].copy()
    c = (mom[:, 1:4].astype(np.float64) + s1 / safe[:, None]) / Q
    nc = (nrm * c).sum(axis=1)
    flip = nc > 0
    nrm[flip], nc[flip] = -nrm[flip], -nc[flip]
    plane_ok = mom[:, 0] >= 3
    have = (edges >= 0).all(axis=1)
    X, good, cos = {}, {}, {}
    for name, col in (("near", 0), ("far", 2)):
        x, y, ok = rays(cam, np.where(have[:, None], edges[:, col:col + 2], 0))
        g = nrm[:, 0] * x + nrm[:, 1] * y + nrm[:, 2]
        length = np.sqrt(x * x + y * y + 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = nc / g
            ok = ok & (np.abs(g) >= 0.1 * length) & (t > 0)
        X[name] = np.stack([t * x, t * y, t], axis=1)
        good[name], cos[name] = ok, np.abs(g) / length
    rays_ok = plane_ok & have & good["near"] & good["far"]
    width = np.where(rays_ok, np.linalg.norm(X["far"] - X["near"], axis=1), 0.0)
    return dict(plane_ok=plane_ok, normal=nrm, offset=-nc, gap=gap, rays_ok=rays_ok, near=X["near"], far=X["far"], width=width,
                cos=np.minimum(cos["near"], cos["far"]))


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def camera(shape):
    """fx = fy = W, the principal point at the centre, the reference's distortion (the cull size covers the image and at
    least four cells of the depth map a side, whatever the image)"""
    h, w = shape
    d = dict(fx=float(w), fy=float(w), cx=w / 2.0, cy=h / 2.0, image_width=w, image_height=h, cull_width=max(w, 56), cull_height=max(h, 56))
    d.update(DISTORTION)
    return d


def wall_cloud(shape, seed, density=0.3, c2w=None):
    """A noisy tilted wall at 2-4 m seen by camera(shape) at the identity pose, about `density` points per pixel, 1 % of them
    pushed beyond 64 m along their ray.  (n, 3) float32 in the world frame of the 3 x 4 c2w (None: camera coordinates)."""
    h, w = shape
    rng = np.random.default_rng(seed)
    n = max(8, int(density * h * w))
    u, v = rng.uniform(0, w, n), rng.uniform(0, h, n)
    x, y = (u - w / 2.0) / w, (v - h / 2.0) / w
    z = 3.0 / (1.0 + 0.55 * x - 0.35 * y) + rng.normal(0, 0.002, n)  # the plane z + 0.55 z x - 0.35 z y = 3
    far = rng.random(n) < 0.01
    z[far] *= 30.0
    p = np.stack([x * z, y * z, z], axis=1)
    if c2w is not None:
        m = np.asarray(c2w, np.float64).reshape(3, 4)
        p = p @ m[:, :3].T + m[:, 3]
    return p.astype(np.float32)


def position_image(shape, seed, density=0.3):
    """(index (H, W) int32, xyz_cam (H, W, 3) float32) without a GPU: every point of wall_cloud lands on the pixel of its
    undistorted projection, the later point wins (any sparse image serves the CPU suite), NaN and far entries included"""
    h, w = shape
    p = wall_cloud(shape, seed, density)
    px = np.floor(p[:, 0] / p[:, 2] * w + w / 2.0).astype(np.int64)
    py = np.floor(p[:, 1] / p[:, 2] * w + h / 2.0).astype(np.int64)
    ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
    index = np.full((h, w), -1, np.int32)
    xyz = np.zeros((h, w, 3), np.float32)
    index[py[ok], px[ok]] = np.flatnonzero(ok).astype(np.int32)
    xyz[py[ok], px[ok]] = p[ok]
    occ = np.flatnonzero(index.ravel() >= 0)
    if len(occ) > 4:  # an occupied pixel whose position is not finite is no member
        xyz.reshape(-1, 3)[occ[len(occ) // 2], 1] = np.nan
    return index, xyz


def deep_wall_image(side=1536, seed=3):
    """every pixel occupied, a wall at 60-63 m: sum q^2 over the image passes 2^64 (2.4e6 pixels x 3 x (62 x 2^16)^2 ~ 1.2e20)"""
    rng = np.random.default_rng(seed)
    xyz = np.empty((side, side, 3), np.float32)
    xyz[..., 0] = rng.uniform(60.0, 63.0, (side, side))
    xyz[..., 1] = rng.uniform(-63.0, -60.0, (side, side))
    xyz[..., 2] = rng.uniform(60.0, 63.0, (side, side))
    index = np.arange(side * side, dtype=np.int32).reshape(side, side)
    return index, xyz


def masks(shape, seed):
    """name -> mask: _mask_edt_ref's generators"""
    return dict(cracks=edt_ref.crack_mask(shape, seed), half=edt_ref.random_mask(shape, 0.5, seed), dense=edt_ref.random_mask(shape, 0.97, seed),
                corner=edt_ref.corner_mask(shape), full=edt_ref.random_mask(shape, 1.0, seed), bytes=edt_ref.byte_mask(shape, seed))


def check_integers(got, mask, index, xyz, threshold, radius, rng_seed=11, budget=600, d2=None, nearest=None):
    """got: dict(flags, edges, w2d2, moments) of the host form or the device; exact equality with the restatement -- flags
    bits 0-3, edges and w2d2 everywhere, the moments at every site (at `budget` seeded sites when there are more)."""
    if d2 is None:
        d2, nearest = edt_ref.edt(mask, threshold)
    flags, edges, w2d2 = integer_stage(mask, d2, nearest, threshold)
    assert np.array_equal(got["flags"] & INTEGER_BITS, flags)
    assert np.array_equal(got["edges"], edges)
    assert np.array_equal(got["w2d2"], w2d2)
    member, q = members(index, xyz)
    ys, xs = np.nonzero(flags & SITE)
    assert not got["moments"][(flags & SITE) == 0].any()
    if len(ys) > budget:
        pick = np.sort(np.random.default_rng(rng_seed).choice(len(ys), budget, replace=False))
        ys, xs = ys[pick], xs[pick]
    want = moments_at(member, q, ys, xs, radius)
    assert np.array_equal(got["moments"][ys, xs], want)
    return flags, want
