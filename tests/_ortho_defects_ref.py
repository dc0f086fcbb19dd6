"""Restatement of the surface defects on ortho maps ("Surface defects on ortho maps", SD2-SD7), written from the
rules and not from the library: int64 integers, truncating division written out (numpy's // floors), window sums from
numpy.cumsum, regions from scipy.ndimage.label with a 3 x 3 structure, ids by numpy.unique of the first pixels.  The suites
compare pcp_ortho_defects_host and the device with it bit for bit.  Also the rasters and the cap scene the suites share."""
import numpy as np
from scipy import ndimage

Q = 1 << 20
OUT = ("kept", "dropped", "hollow_pixels", "bulge_pixels", "unsupported", "refused", "first_pass", "surface")
(R_CLASS, R_PIXELS, R_MEASURED, R_SUM, R_MAX, R_MAX_PIXEL, R_COL_MIN, R_COL_MAX, R_ROW_MIN, R_ROW_MAX, R_SUM_COL, R_SUM_ROW, R_OPEN,
 R_FIRST, R_FIRST_PASS, R_ZERO) = range(16)


def trunc_div(e, n):
    """C's division of int64 arrays (n > 0)"""
    return np.sign(e) * (np.abs(e) // n)


def quanta(depth, status):
    """SD2: (surface bool, refused bool, q int64)"""
    depth = np.asarray(depth, np.float32)
    has = (status == 1) | (status == 2)
    with np.errstate(invalid="ignore"):
        fine = np.isfinite(depth) & (np.abs(depth) <= np.float32(512.0))
    surface = has & fine
    q = np.zeros(depth.shape, np.int64)
    q[surface] = np.rint(depth[surface].astype(np.float64) * Q).astype(np.int64)  # (exact scaling; rint: ties to even)
    return surface, has & ~fine, q


def window_sums(a, W):
    """the sum of int64 `a` over rows r - W .. r + W, columns c - W .. c + W clipped to the raster"""
    h, w = a.shape
    t = np.zeros((h + 1, w + 1), np.int64)
    t[1:, 1:] = np.cumsum(np.cumsum(a, axis=0), axis=1)
    r0 = np.clip(np.arange(h) - W, 0, h)[:, None]
    r1 = np.clip(np.arange(h) + W + 1, 0, h)[:, None]
    c0 = np.clip(np.arange(w) - W, 0, w)[None, :]
    c1 = np.clip(np.arange(w) + W + 1, 0, w)[None, :]
    return t[r1, c1] - t[r0, c1] - t[r1, c0] + t[r0, c0]


def _pass(q, member, surface, W, T, min_support):
    """SD3 over the pixels of `member`: (supported, dev, class with every bit on) at the surface pixels"""
    S = window_sums(np.where(member, q, 0), W)
    n = window_sums(member.astype(np.int64), W)
    ok = surface & (n >= min_support)
    e = np.where(ok, q * n - S, 0)
    dev = np.where(ok, trunc_div(e, np.maximum(n, 1)), 0)
    cls = np.where(ok & (e >= T * n), 1, np.where(ok & (e <= -T * n), 2, 0))
    return ok, dev, cls


def defects(depth, status, threshold=0.002, window=0, refine=False, min_support=1, min_pixels=1, classes=3):
    """dict(out (8 int64), dev int32, cls uint8, region int32, rows (N, 16) int64) as pcp_ortho_defects_host returns them"""
    depth = np.asarray(depth, np.float32)
    status = np.asarray(status, np.uint8)
    h, w = depth.shape
    T = int(np.rint(np.float64(np.float32(threshold)) * Q))
    surface, refused, q = quanta(depth, status)
    first_pass = np.zeros((h, w), bool)
    unsupported = 0
    if window == 0:  # SD3b
        dev = q.copy()
        cls = np.where(surface & (q >= T), 1, np.where(surface & (q <= -T), 2, 0))
    else:
        ok, dev, cls = _pass(q, surface, surface, window, T, min_support)
        unsupported = int((surface & ~ok).sum())
        if refine:  # SD4
            ok2, dev2, cls2 = _pass(q, surface & (cls == 0), surface, window, T, min_support)
            dev = np.where(ok2, dev2, dev)
            cls = np.where(ok2, cls2, cls)
            first_pass = surface & ~ok2
    cls = np.where((cls == 1) & bool(classes & 1), 1, np.where((cls == 2) & bool(classes & 2), 2, 0)).astype(np.uint8)
    # SD5
    lab = np.zeros((h, w), np.int64)
    base = 0
    for k in (1, 2):
        l, cnt = ndimage.label(cls == k, structure=np.ones((3, 3), int))
        lab = np.where(l > 0, l + base, lab)
        base += cnt
    flat = lab.ravel()
    ids, first = np.unique(flat, return_index=True)
    first = first[ids > 0]
    ids = ids[ids > 0]
    sizes = np.bincount(flat, minlength=base + 1)[ids]
    keep = sizes >= min_pixels
    order = np.argsort(first[keep])
    kept_ids = ids[keep][order]
    n_rows = len(kept_ids)
    number = np.zeros(base + 1, np.int64)
    number[kept_ids] = np.arange(1, n_rows + 1)
    region = number[lab]
    # SD7
    rows = np.zeros((n_rows, 16), np.int64)
    inside = region.ravel() > 0
    pix = np.flatnonzero(inside)
    row_of = region.ravel()[pix] - 1
    rr, cc = pix // w, pix % w
    absdev = np.abs(dev.ravel()[pix])
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = surface
    closed = pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]  # (the raster's edge has a neighbour outside)
    open_px = ~closed.ravel()[pix]

    def total(v):
        return np.bincount(row_of, weights=None if v is None else v, minlength=n_rows)

    if n_rows:
        rows[:, R_PIXELS] = total(None)
        rows[:, R_MEASURED] = np.bincount(row_of[status.ravel()[pix] == 1], minlength=n_rows)
        rows[:, R_OPEN] = np.bincount(row_of[open_px], minlength=n_rows)
        rows[:, R_FIRST_PASS] = np.bincount(row_of[first_pass.ravel()[pix]], minlength=n_rows)
        for col, v in ((R_SUM, absdev), (R_SUM_COL, cc), (R_SUM_ROW, rr)):
            s = np.zeros(n_rows, np.int64)
            np.add.at(s, row_of, v)
            rows[:, col] = s
        for col, v, f, start in ((R_COL_MIN, cc, np.minimum, w), (R_COL_MAX, cc, np.maximum, -1), (R_ROW_MIN, rr, np.minimum, h),
                                 (R_ROW_MAX, rr, np.maximum, -1)):
            s = np.full(n_rows, start, np.int64)
            f.at(s, row_of, v)
            rows[:, col] = s
        # the greatest |dev| and the lowest pixel among equals: pixels ascend, so a stable sort by -|dev| puts it first
        o = np.lexsort((pix, -absdev, row_of))
        lead = np.concatenate([[True], row_of[o][1:] != row_of[o][:-1]])
        rows[:, R_MAX] = absdev[o][lead]
        rows[:, R_MAX_PIXEL] = pix[o][lead]
        fp = np.full(n_rows, h * w, np.int64)
        np.minimum.at(fp, row_of, pix)
        rows[:, R_FIRST] = fp
        rows[:, R_CLASS] = cls.ravel()[fp]
    out = np.array([n_rows, len(ids) - n_rows, (cls == 1).sum(), (cls == 2).sum(), unsupported, refused.sum(), first_pass.sum(),
                    surface.sum()], np.int64)
    return dict(out=out, dev=dev.astype(np.int32), cls=cls, region=region.astype(np.int32), rows=rows)


def same(got, want):
    """None, or the name of the first part that differs"""
    for k in ("out", "dev", "cls", "region", "rows"):
        if got[k].shape != want[k].shape or not np.array_equal(got[k], want[k]):
            return k
    return None


# ---- the rasters --------------------------------------------------------------------------------------------------------------
def random_field(h, w, seed, empty=0.04, filled=0.03, odd=True):
    """(depth float32, status uint8): a smooth random surface of a few millimetres with sharp hollows and bulges of both classes,
    a few per cent of empty and of filled pixels, and (odd) NaN and 600 m depths for SD2"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    depth = 0.003 * np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0) + rng.normal(0, 0.0008, (h, w))
    for _ in range(max(2, h * w // 900)):
        r, c = rng.integers(0, h), rng.integers(0, w)
        rad = rng.integers(1, 7)
        sign = 1.0 if rng.random() < 0.5 else -1.0
        m = (yy - r) ** 2 + (xx - c) ** 2 <= rad * rad
        depth[m] += sign * rng.uniform(0.004, 0.02)
    depth = depth.astype(np.float32)
    u = rng.random((h, w))
    status = np.where(u < empty, 0, np.where(u < empty + filled, 2, 1)).astype(np.uint8)
    if odd and h * w >= 16:
        k = rng.choice(h * w, size=min(6, h * w // 8), replace=False)
        depth.ravel()[k[::2]] = np.nan
        depth.ravel()[k[1::2]] = 600.0
    return depth, status


def flat(h, w, value=0.0):
    return np.full((h, w), value, np.float32), np.ones((h, w), np.uint8)


def diagonal(h=129, w=131, d=0.01):
    """one-pixel diagonals from the two upper corners downwards, joined only across corners (NW and NE links, hence across tile
    corners); they share pixel (65, 65): one region of 2 h - 1 pixels"""
    depth, status = flat(h, w)
    rows = np.arange(h)
    depth[rows, rows] = d
    depth[rows, w - 1 - rows] = d
    return depth, status


def tile_corners(h=40, w=131, d=0.01):
    """links across the exact corners of 32 x 16 tiles: (16, 31) -- (15, 32) is a NE link from a pixel that lies on its tile's top
    row and right column at once; (32, 64) -- (31, 63) a NW link from a tile's first pixel; an anti-diagonal from (0, 111) down
    whose pixel (16, 95) is such a corner pixel too; and a bulge pair across a corner that must not join the hollows"""
    depth, status = flat(h, w)
    depth[16, 31] = depth[15, 32] = d
    depth[32, 64] = depth[31, 63] = d
    rows = np.arange(h)
    depth[rows, 111 - rows] = d
    depth[16, 63] = depth[15, 64] = -d
    return depth, status


def spiral(h=129, w=131, d=0.01):
    """a one-pixel spiral filling the raster with one empty lane between its turns: the long chain"""
    depth, status = flat(h, w)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    r, c = 0, 0
    path = []
    while top <= bottom and left <= right:
        for c in range(left, right + 1):
            path.append((top, c))
        for r in range(top + 1, bottom + 1):
            path.append((r, right))
        if bottom > top:
            for c in range(right - 1, left - 1, -1):
                path.append((bottom, c))
        if right > left:
            for r in range(bottom - 1, top + 1, -1):
                path.append((r, left))
        if bottom - top >= 2 and right - left >= 2:  # the way in to the next turn
            path.append((top + 2, left))
            path.append((top + 2, left + 1))
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    rr, cc = np.array(path).T
    depth[rr, cc] = d
    return depth, status


def checkerboard(h=37, w=41, d=0.01):
    depth, status = flat(h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    depth[:] = np.where((yy + xx) % 2 == 0, d, -d)
    return depth, status


def reversed_sizes(h=40, w=70, d=0.01):
    """two regions whose first pixels are in reverse order of their sizes: a small one first, a large one after it"""
    depth, status = flat(h, w)
    depth[2:4, 50:53] = d
    depth[10:30, 5:40] = d
    return depth, status


def sized(min_pixels, h=30, w=64, d=0.01):
    """one region of min_pixels - 1 pixels and one of min_pixels, both rows of single pixels"""
    depth, status = flat(h, w)
    depth[5, 3:3 + min_pixels - 1] = d
    depth[15, 3:3 + min_pixels] = -d
    return depth, status


def equal_maxima(h=24, w=30):
    depth, status = flat(h, w)
    depth[8:12, 6:20] = 0.005
    depth[10, 17] = 0.02
    depth[9, 8] = 0.02
    depth[11, 7] = 0.02
    return depth, status


def edge_and_hole(h=40, w=50, d=0.01):
    """a region touching the raster's edge and one around a hole of empty pixels"""
    depth, status = flat(h, w)
    depth[0:5, 10:18] = d
    depth[20:32, 20:36] = -d
    status[24:27, 26:30] = 0
    status[29, 22] = 2
    return depth, status


# ---- the cap scene ------------------------------------------------------------------------------------------------------------
CAP_A, CAP_H, CAP_T = 0.05, 0.012, 0.002
CAP_RS = (CAP_A ** 2 + CAP_H ** 2) / (2 * CAP_H)
CAP_AT = float(np.sqrt(CAP_RS ** 2 - (CAP_RS - CAP_H + CAP_T) ** 2))
CAP_AREA = float(np.pi * CAP_AT ** 2)
CAP_VOLUME = float(np.pi * (CAP_H - CAP_T) * (3 * CAP_AT ** 2 + (CAP_H - CAP_T) ** 2) / 6 + np.pi * CAP_AT ** 2 * CAP_T)
CAP_CENTRES = ((0.17, 0.25), (0.43, 0.25))  # hollow, bulge


def cap_spacing(gsd):
    """the lattice of the scene at this gsd: half a pixel, four points a pixel (the map keeps the nearest of them)"""
    return gsd / 2


def cap_scene(gsd, seed=7):
    """A planar wall of 0.6 x 0.5 m in z = 0 on a jittered lattice of half the gsd, seen along +z, with one spherical-cap
    hollow (z > 0: away from the viewer) and one bulge: (n, 3) float32"""
    rng = np.random.default_rng(seed)
    s = cap_spacing(gsd)
    x, y = np.meshgrid(np.arange(s / 2, 0.6, s), np.arange(s / 2, 0.5, s))
    x = (x + rng.uniform(-0.4 * s, 0.4 * s, x.shape)).ravel()
    y = (y + rng.uniform(-0.4 * s, 0.4 * s, y.shape)).ravel()
    z = np.zeros_like(x)
    for (cx, cy), sign in zip(CAP_CENTRES, (1.0, -1.0)):
        r2 = (x - cx) ** 2 + (y - cy) ** 2
        m = r2 <= CAP_A ** 2
        z[m] = sign * (np.sqrt(CAP_RS ** 2 - r2[m]) - (CAP_RS - CAP_H))
    return np.stack([x, y, z], axis=1).astype(np.float32)


def cap_frame(gsd):
    """the wall's frame, given exactly: u = +x, v = +y, n = +z (u x v = n), the raster over the whole wall"""
    return dict(o=(0.0, 0.0, 0.0), u=(1.0, 0.0, 0.0), v=(0.0, 1.0, 0.0), n=(0.0, 0.0, 1.0), gsd=gsd, width=int(round(0.6 / gsd)),
                height=int(round(0.5 / gsd)), d_min=-0.1, d_max=0.1)


def cap_measures(rows, gsd):
    """per region: (class, area m^2, volume m^3, greatest depth m)"""
    return [(int(r[R_CLASS]), r[R_PIXELS] * gsd * gsd, r[R_SUM] / Q * gsd * gsd, r[R_MAX] / Q) for r in rows]


def cap_bounds(gsd):
    """(area band, relative volume bound, depth bound): two pixel footprints along the boundary; 10 % at 4 mm and 5 % at 2 mm
    (first order in gsd: the map keeps the nearest point of a pixel); one lattice spacing's worth of the cap's steepest slope"""
    slope = CAP_A / np.sqrt(CAP_RS ** 2 - CAP_A ** 2)
    return 2 * np.pi * CAP_AT * 2 * gsd, {0.004: 0.10, 0.002: 0.05}[gsd], cap_spacing(gsd) * slope


# ---- the cases the CPU and the GPU suites share: (name, raster, keywords) ----------------------------------------------------
def cases():
    out = []
    for (h, w), windows in (((1, 1), (0, 1)), ((1, 257), (0, 1)), ((257, 1), (0, 1)), ((3, 67), (1, 7)), ((202, 242), (0, 7, 40)),
                            ((260, 300), (1024,))):
        for W in windows:
            for refine in ((False, True) if (h, w) == (202, 242) and W > 0 else (False,)):
                out.append((f"random-{w}x{h}-W{W}-r{int(refine)}", ("random", h, w),
                            dict(window=W, refine=refine, min_support=3 if W else 1, min_pixels=2)))
    out.append(("random-70x60-W5-support20-bulges", ("random", 60, 70), dict(window=5, refine=True, min_support=20, classes=2)))
    out.append(("diagonal", ("diagonal",), {}))
    out.append(("tile-corners", ("tile_corners",), {}))
    out.append(("spiral", ("spiral",), {}))
    out.append(("checkerboard", ("checkerboard",), {}))
    out.append(("checkerboard-hollows", ("checkerboard",), dict(classes=1)))
    out.append(("reversed-sizes", ("reversed_sizes",), {}))
    out.append(("min-pixels", ("sized", 5), dict(min_pixels=5)))
    out.append(("equal-maxima", ("equal_maxima",), {}))
    out.append(("edge-and-hole", ("edge_and_hole",), {}))
    out.append(("no-defects", ("flat", 20, 33, 0.001), {}))
    return out


def raster(spec):
    """(depth, status) of a case's raster"""
    if spec[0] == "random":
        return random_field(spec[1], spec[2], spec[1] * 1000 + spec[2])
    return globals()[spec[0]](*spec[1:])
