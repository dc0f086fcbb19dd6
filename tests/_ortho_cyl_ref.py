"""The unrolled maps of cylindrical facets restated in numpy ("Cylindrical facets", CY1-CY6), for
test_ortho_cyl_cpu.py and test_ortho_cyl_gpu.py: written from the rules, not by calling the library.  CY2 with explicit float32
and float64 casts, CY3 operation by operation, the winner and the fill as _ortho_ref's, the fit with numpy.linalg.eigh and
lstsq; and the scenes of the tests."""
import numpy as np

import _ortho_ref as oref

F32 = np.float32
F64 = np.float64
PI4 = F64(np.pi) / F64(4)   # the doubles nearest pi/4, pi/2, pi, 2 pi (exact scalings of the double nearest pi)
PI2 = F64(np.pi) / F64(2)
PI = F64(np.pi)
TWO_PI = F64(np.pi) * F64(2)
T8 = F64(float.fromhex("0x1.a827999fcef32p-2"))
COEF = [F64((-1.0) ** k) / F64(2 * k + 1) for k in range(13)]  # the doubles nearest (-1)^k / (2k + 1): a correctly rounded quotient
BINS = 4096


def frame(c, a, e, b, radius, gsd, width, height, d_min, d_max, side):
    r = lambda v: [float(F32(x)) for x in v]
    return dict(c=r(c), a=r(a), e=r(e), b=r(b), radius=float(F32(radius)), gsd=float(F32(gsd)), width=int(width), height=int(height),
                d_min=float(F32(d_min)), d_max=float(F32(d_max)), side=int(side))


def angle(S, T):
    """CY3: theta in [0, 2 pi] of fp64 pairs, operation by operation"""
    S = np.asarray(S, F64)
    T = np.asarray(T, F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        x, y = np.abs(S), np.abs(T)
        steep = y > x
        m, M = np.where(steep, x, y), np.where(steep, y, x)
        q = m / M
        far = q > T8
        r = np.where(far, (q - F64(1)) / (q + F64(1)), q)
        base = np.where(far, PI4, F64(0))
        z = r * r
        P = np.full(z.shape, COEF[12], F64)
        for k in range(11, -1, -1):
            P = P * z + COEF[k]
        phi = base + r * P
        phi = np.where(steep, PI2 - phi, phi)
        phi = np.where(S < 0, PI - phi, phi)
        phi = np.where(T < 0, TWO_PI - phi, phi)
    return phi


def coords(fr, xyz):
    """CY2 before the tests: (usable, x, y, depth) as float32 per row"""
    p = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    c = np.asarray(fr["c"], F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = (p - c).astype(F32)

        def dot(v):
            v = np.asarray(v, F32)
            return ((d[:, 0] * v[0]).astype(F32) + ((d[:, 1] * v[1]).astype(F32) + (d[:, 2] * v[2]).astype(F32)).astype(F32)).astype(F32)

        inv = F32(F32(1.0) / F32(fr["gsd"]))
        s, t, h = dot(fr["e"]), dot(fr["b"]), dot(fr["a"])
        S, T = s.astype(F64), t.astype(F64)
        rho = np.sqrt(S * S + T * T)
        R = F64(F32(fr["radius"]))
        arc = R * angle(S, T)
        x = (arc * F64(inv)).astype(F32)
        y = (h * inv).astype(F32)
        depth = (F64(fr["side"]) * (rho - R)).astype(F32)
        ok = np.isfinite(p).all(axis=1) & (rho > 0)
    return ok, x, y, depth


def project(fr, xyz):
    """CY2: (contributor mask, pixel, depth) of every row; the has bit is the caller's"""
    ok, x, y, depth = coords(fr, xyz)
    with np.errstate(invalid="ignore"):
        ok = ok & (x >= F32(0)) & (x < F32(fr["width"])) & (y >= F32(0)) & (y < F32(fr["height"]))
        ok &= (depth >= F32(fr["d_min"])) & (depth <= F32(fr["d_max"]))
        col = np.floor(np.where(ok, x, 0)).astype(np.int32)
        row = np.floor(np.where(ok, y, 0)).astype(np.int32)
        depth = np.where(depth == 0, F32(0), depth).astype(F32)  # -0 counts as +0
    return ok, row.astype(np.int64) * fr["width"] + col, depth


def cuts(fr, xyz):
    """how many finite rows off the axis the raster and the depth window cut: (by the raster, by the window alone)"""
    ok, x, y, depth = coords(fr, xyz)
    with np.errstate(invalid="ignore"):
        inside = (x >= F32(0)) & (x < F32(fr["width"])) & (y >= F32(0)) & (y < F32(fr["height"]))
        window = (depth >= F32(fr["d_min"])) & (depth <= F32(fr["d_max"]))
    return int((ok & ~inside).sum()), int((ok & inside & ~window).sum())


def winners(fr, xyz, has=None, index_base=0):
    """OM3 on CY2's pixels: _ortho_ref.winners with the cylinder's projection"""
    ok, pixel, depth = project(fr, xyz)
    if has is not None:
        ok &= np.asarray(has).astype(bool)
    rows = np.flatnonzero(ok)
    g = (rows + index_base).astype(np.uint64)
    o = oref.ord_bits(depth[rows].view(np.uint32))
    order = np.lexsort((g, o, pixel[rows]))
    px = pixel[rows][order]
    first = np.ones(len(px), bool)
    first[1:] = px[1:] != px[:-1]
    starts = np.flatnonzero(first)
    per_pixel = np.diff(np.append(starts, len(px)))
    os_ = o[order]
    same_as_first = os_ == np.repeat(os_[starts], per_pixel)
    ties = int((np.add.reduceat(same_as_first.astype(np.int64), starts) >= 2).sum()) if len(starts) else 0
    win = rows[order][first]
    return dict(pixel=px[first], row=win, depth=depth[win], contributors=len(rows), per_pixel=per_pixel, ties=ties)


def ortho(fr, xyz, rgb, label=None, has=None, index_base=0, fill_radius=0):
    """CY2-CY4: dict(index, depth, rgb[, label], status, source, contributors, occupied, filled, per_pixel, ties)"""
    h, w = fr["height"], fr["width"]
    win = winners(fr, xyz, has, index_base)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    index = np.full(h * w, oref.EMPTY_INDEX, np.uint32)
    depth = np.zeros(h * w, F32)
    colour = np.zeros((h * w, 3), np.uint8)
    lab = np.zeros(h * w, np.uint8)
    index[win["pixel"]] = (win["row"] + index_base).astype(np.uint32)
    depth[win["pixel"]] = win["depth"]
    colour[win["pixel"]] = rgb[win["row"]]
    if label is not None:
        lab[win["pixel"]] = np.asarray(label, np.uint8)[win["row"]]
    occupied = np.zeros(h * w, bool)
    occupied[win["pixel"]] = True
    source = oref.fill_sources(occupied.reshape(h, w), fill_radius).reshape(-1)  # (no wrap across the seam: CY4)
    status = np.where(source < 0, 0, np.where(occupied, 1, 2)).astype(np.uint8)
    take = np.where(source < 0, 0, source)
    got = source >= 0
    out = dict(index=np.where(got, index[take], oref.EMPTY_INDEX).astype(np.uint32).reshape(h, w),
               depth=np.where(got, depth[take], F32(0)).astype(F32).reshape(h, w),
               rgb=np.where(got[:, None], colour[take], 0).astype(np.uint8).reshape(h, w, 3),
               status=status.reshape(h, w), source=source.reshape(h, w),
               contributors=win["contributors"], occupied=int(occupied.sum()), filled=int((status == 2).sum()),
               per_pixel=win["per_pixel"], ties=win["ties"])
    if label is not None:
        out["label"] = np.where(got, lab[take], 0).astype(np.uint8).reshape(h, w)
    return out


same = oref.same


# ---- CY6 ------------------------------------------------------------------------------------------------------------------
def fit(xyz, normal, gsd, has=None, viewer=None):
    """CY6 with eigh and lstsq: (frame dict, dict(rows, rms, dev_min, dev_max, arc, ev0, ev1, ev2, closed)); the fp64
    values before the frame's casts ride along as c0 (axis point at the centroid's height), axis, R."""
    p32 = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n32 = np.ascontiguousarray(normal, F32).reshape(-1, 3)
    use = np.isfinite(p32).all(axis=1) & np.isfinite(n32).all(axis=1) & (n32 != 0).any(axis=1)
    if has is not None:
        use &= np.asarray(has).astype(bool)
    p, nn = p32[use].astype(F64), n32[use].astype(F64)
    cnt = len(p)
    assert cnt >= 16
    ev, vec = np.linalg.eigh(nn.T @ nn / cnt)
    assert ev[1] > 1e-4 * ev[2]
    a = vec[:, 0]
    if a[np.argmax(np.abs(a))] > 0:
        a = -a
    least = int(np.argmin(np.abs(a)))
    e0 = np.eye(3)[least] - a[least] * a
    e0 /= np.linalg.norm(e0)
    g0 = np.cross(a, e0)
    cen = p.mean(axis=0)
    d = p - cen
    u, v = d @ e0, d @ g0
    sol = np.linalg.lstsq(np.stack([u, v, np.ones(cnt)], axis=1), -(u * u + v * v), rcond=None)[0]
    uc, vc = -0.5 * sol[0], -0.5 * sol[1]
    R = np.sqrt(uc * uc + vc * vc - sol[2])
    c0 = cen + uc * e0 + vc * g0
    side = -1
    if viewer is not None:
        w = np.asarray(viewer, F64) - c0
        if w @ w - (w @ a) ** 2 <= R * R:
            side = 1
    b0 = side * g0
    d = p - c0
    s, t, hh = d @ e0, d @ b0, d @ a
    rho = np.sqrt(s * s + t * t)
    dev = rho - R
    g = float(F32(gsd))
    width_bin = TWO_PI / BINS
    occ = np.zeros(BINS, bool)
    occ[np.minimum(BINS - 1, np.floor(angle(s, t)[rho > 0] / width_bin).astype(np.int64))] = True
    first = int(np.flatnonzero(occ)[0])
    best, best_next, run = 0, 0, 0
    for k in range(1, BINS + 1):
        pos = (first + k) % BINS
        if not occ[pos]:
            run += 1
        else:
            if run > best:
                best, best_next = run, pos
            run = 0
    gap = best * width_bin
    closed = bool(gap * R < 2.0 * g)
    if closed:
        e = e0
    else:
        seam = best_next * width_bin - g / R
        e = np.cos(seam) * e0 + np.sin(seam) * b0
    b = side * np.cross(a, e)
    fr = frame(c0 + (hh.min() - g) * a, a, e, b, R, gsd, 1, 1, 0.0, 1.0, side)
    ok, x, y, depth = coords(fr, p32[use])
    around = TWO_PI * F64(F32(R))
    fr["width"] = int(max(np.ceil(around / g), np.floor(x[ok].max()) + 1)) if closed else int(np.floor(x[ok].max())) + 2
    if closed and fr["width"] * g > around + g:  # (CY1 would refuse the wider raster: the row at 2 pi stays outside)
        fr["width"] = int(np.ceil(around / g))
    fr["height"] = int(np.floor(y[ok].max())) + 2
    fr["d_min"] = float(F32(depth[ok].min() - F32(gsd)))
    fr["d_max"] = float(F32(depth[ok].max() + F32(gsd)))
    stats = dict(rows=cnt, rms=float(np.sqrt((dev * dev).sum() / cnt)), dev_min=float(dev.min()), dev_max=float(dev.max()),
                 arc=float(TWO_PI - gap), ev0=float(ev[0]), ev1=float(ev[1]), ev2=float(ev[2]), closed=closed, c0=c0, axis=a, R=float(R))
    return fr, stats


# ---- the scenes -------------------------------------------------------------------------------------------------------------
CENTRE = np.array([3.0, -2.0, 1.0])


def rotation(seed):
    """a proper rotation: QR of a seeded normal matrix, determinant made +1"""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def cylinder_scene(N, R, H, arc, sigma, seed):
    """N points of a cylinder of radius R and height H over the angles [0, arc): uniform (theta, h), Gaussian radial noise
    sigma, rotated by rotation(seed) and centred at CENTRE, cast to float32.  dict(xyz, axis (the rotated z), centre, R, theta,
    h, rot, outward (the exact unit normals, float32))"""
    rng = np.random.default_rng(seed)
    theta = rng.random(N) * arc
    h = (rng.random(N) - 0.5) * H
    rad = R + sigma * rng.normal(size=N)
    rot = rotation(seed)
    out = np.stack([np.cos(theta), np.sin(theta), np.zeros(N)], axis=1)
    local = out * rad[:, None] + np.stack([np.zeros(N), np.zeros(N), h], axis=1)
    xyz = (local @ rot.T + CENTRE).astype(F32)
    return dict(xyz=xyz, axis=rot[:, 2].copy(), centre=CENTRE.copy(), R=R, theta=theta, h=h, rot=rot, outward=(out @ rot.T).astype(F32))


def pca_normals(xyz, radius):
    """a normal per point: the eigenvector of the smallest eigenvalue of the covariance of its neighbours within `radius`"""
    from scipy.spatial import cKDTree

    p = np.asarray(xyz, F64)
    tree = cKDTree(p)
    out = np.zeros((len(p), 3), F32)
    for i, nb in enumerate(tree.query_ball_point(p, radius)):
        if len(nb) < 3:
            continue
        q = p[nb] - p[nb].mean(axis=0)
        out[i] = np.linalg.eigh(q.T @ q)[1][:, 0]
    return out


def hash_colours(n):
    return oref.hash_colours(n)


def words_of(rgb, has=None):
    w = rgb[:, 0].astype(np.uint32) | (rgb[:, 1].astype(np.uint32) << 8) | (rgb[:, 2].astype(np.uint32) << 16)
    return w | (np.uint32(1 << 24) if has is None else (np.asarray(has, np.uint32) << 24))
