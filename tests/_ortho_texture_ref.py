"""The orthophoto restated in numpy ("Orthophotos", OT2-OT6), for test_ortho_texture_*.py.  OT3 with explicit float32
casts; OT4-OT5 from oracle.np_oracle's pose_to_matrices, cull_frame (the depth maps of the cloud), project_frame on the surface
points, the keep rule ~(range64 > dmap[cell] + slack) and scores; a stable sort by descending score; fp32 sums as
np_oracle.colorize writes them."""
import numpy as np

from oracle import np_oracle as npo

F32 = np.float32
LAYERS = ("rgb", "mask", "status", "view", "count")
COUNTS = ("surface", "textured", "unseen")


def _rect(fr, rect):
    return (0, 0, fr["width"], fr["height"]) if rect is None else tuple(int(v) for v in rect)


def surface(fr, source, depth, k, interpolate=True, max_step=0.05, rect=None):
    """OT3: (ok (h k, w k) bool, xyz (h k, w k, 3) float32, zeros where there is no surface)"""
    W, H = fr["width"], fr["height"]
    x0, y0, w, h = _rect(fr, rect)
    source = np.asarray(source, np.int32).reshape(H, W)
    dflat = np.asarray(depth, F32).reshape(-1)
    Xg, Yg = np.meshgrid(x0 * k + np.arange(w * k, dtype=np.int64), y0 * k + np.arange(h * k, dtype=np.int64))
    c, r = Xg // k, Yg // k
    src = source[r, c]
    ok = src >= 0
    d00 = dflat[np.where(ok, src, 0)]
    d = d00
    if interpolate:
        a, b = 2 * (Xg % k) + 1 - k, 2 * (Yg % k) + 1 - k
        c2, r2 = c + np.sign(a), r + np.sign(b)
        inside = (c2 >= 0) & (c2 < W) & (r2 >= 0) & (r2 < H)
        c2, r2 = np.clip(c2, 0, W - 1), np.clip(r2, 0, H - 1)

        def neighbour(rr, cc):
            s = source[rr, cc]
            dn = dflat[np.where(s >= 0, s, 0)]
            return (s >= 0) & (np.abs((dn - d00).astype(F32)) <= F32(max_step)), dn

        g10, d10 = neighbour(r, c2)
        g01, d01 = neighbour(r2, c)
        g11, d11 = neighbour(r2, c2)
        # every neighbour the interpolation READS: (c', r) unless a == 0, (c, r') unless b == 0, (c', r') unless either is 0
        take = ok & inside & ((a == 0) | g10) & ((b == 0) | g01) & ((a == 0) | (b == 0) | g11)
        d10 = np.where(a == 0, d00, d10)
        d11 = np.where(a == 0, d01, d11)
        d01 = np.where(b == 0, d00, d01)
        d11 = np.where(b == 0, d10, d11)
        wx = (np.abs(a).astype(F32) / F32(2 * k)).astype(F32)
        wy = (np.abs(b).astype(F32) / F32(2 * k)).astype(F32)
        top = (d00 + (wx * (d10 - d00).astype(F32)).astype(F32)).astype(F32)
        bot = (d01 + (wx * (d11 - d01).astype(F32)).astype(F32)).astype(F32)
        d = np.where(take, (top + (wy * (bot - top).astype(F32)).astype(F32)).astype(F32), d00).astype(F32)
    gk = F32(F32(fr["gsd"]) / F32(k))
    s = ((Xg.astype(F32) + F32(0.5)).astype(F32) * gk).astype(F32)
    t = ((Yg.astype(F32) + F32(0.5)).astype(F32) * gk).astype(F32)
    xyz = np.zeros(ok.shape + (3,), F32)
    for ax in range(3):
        o, u, v, n = (F32(fr[key][ax]) for key in ("o", "u", "v", "n"))
        plane = ((s * u).astype(F32) + (t * v).astype(F32)).astype(F32)
        xyz[..., ax] = np.where(ok, (o + (plane + (d * n).astype(F32)).astype(F32)).astype(F32), F32(0))
    return ok, xyz


def depth_maps(cam, poses, x, y, z):
    """the z-buffer depth maps of a cloud, one (mh * mw) float32 row per keyframe, and the keyframes' w2c"""
    w2cs, maps = [], []
    for pose in poses:
        w2c, _ = npo.pose_to_matrices(pose)
        _, dmap, _ = npo.cull_frame(cam, w2c, x, y, z)
        w2cs.append(w2c)
        maps.append(dmap.reshape(-1))
    return w2cs, np.stack(maps)


def gained(c, g):
    """EG5's c' of a channel (uint8 array) under gain g: fl32 product, fl32 sum with 0.5, truncation, clamp"""
    v = ((c.astype(F32) * F32(g)).astype(F32) + F32(0.5)).astype(F32)
    return np.minimum(v.astype(np.int32), 255).astype(np.uint8)


def texture(cam, poses, images, masks, w2cs, dmaps, fr, source, depth, k, views=1, interpolate=True, max_step=0.05, rect=None, gains=None,
            slack=0.05):
    """OT3-OT6 over every keyframe: dict(rgb, mask, status, view, count, surface, textured, unseen, two_or_more, refused_by_keep,
    five_or_more, six_or_more); masks: a list of (H, W) uint8 or None (no mask uploaded)"""
    ok, xyz = surface(fr, source, depth, k, interpolate, max_step, rect)
    shape = ok.shape
    sel = np.flatnonzero(ok.ravel())
    pts = xyz.reshape(-1, 3)[sel]
    n, nf = len(sel), len(poses)
    score = np.full((nf, n), -np.inf, F32)
    texel = np.zeros((nf, n, 3), np.uint8)  # r, g, b
    mbyte = np.zeros((nf, n), np.uint8)
    refused = np.zeros(n, bool)
    for f, pose in enumerate(poses):
        p = npo.project_frame(cam, w2cs[f], pts[:, 0], pts[:, 1], pts[:, 2])
        cell = p["cell"]
        keep = np.zeros(n, bool)
        inmap = cell >= 0
        keep[inmap] = ~(p["range64"][inmap] > dmaps[f][cell[inmap]].astype(np.float64) + slack)
        listed = keep & (p["pixel"] >= 0)
        refused |= inmap & ~keep & (p["pixel"] >= 0)  # in the image, in the depth map, hidden by it
        _, _, fin = npo.scores(p["xc"], p["yc"], p["zc"], pose)
        score[f, listed] = fin[listed]
        px = p["pixel"][listed]
        bgr = np.asarray(images[f], np.uint8).reshape(-1, 3)[px]
        rgb = bgr[:, ::-1]
        if gains is not None:
            rgb = gained(rgb, gains[f])
        texel[f, listed] = rgb
        if masks is not None and masks[f] is not None:
            mbyte[f, listed] = np.asarray(masks[f], np.uint8).reshape(-1)[px]
    count = np.isfinite(score).sum(axis=0)
    order = np.argsort(-score, axis=0, kind="stable")  # descending score, ties keep ascending keyframe order
    cols = np.arange(n)
    tot = np.zeros(n, F32)
    acc = np.zeros((n, 3), F32)
    for j in range(min(views, nf)):
        fj = order[j]
        use = j < np.minimum(count, views)
        s = np.where(use, score[fj, cols], F32(0)).astype(F32)
        for ch in range(3):
            acc[:, ch] = np.where(use, (acc[:, ch] + (texel[fj, cols, ch].astype(F32) * s).astype(F32)).astype(F32), acc[:, ch])
        tot = np.where(use, (tot + s).astype(F32), tot)
    textured = count >= 1
    with np.errstate(invalid="ignore", divide="ignore"):
        rgb = np.where(textured[:, None], (acc / tot[:, None]).astype(F32), F32(0)).astype(np.int64).astype(np.uint8)
    out = dict(rgb=np.zeros(shape + (3,), np.uint8), mask=np.zeros(shape, np.uint8), status=np.zeros(shape, np.uint8),
               view=np.full(shape, -1, np.int16), count=np.zeros(shape, np.uint8))
    out["rgb"].reshape(-1, 3)[sel] = rgb
    out["mask"].reshape(-1)[sel] = np.where(textured, mbyte[order[0], cols], 0)
    out["status"].reshape(-1)[sel] = np.where(textured, 1, 2)
    out["view"].reshape(-1)[sel] = np.where(textured, order[0], -1)
    out["count"].reshape(-1)[sel] = np.minimum(count, 255)
    out.update(surface=n, textured=int(textured.sum()), unseen=int(n - textured.sum()), two_or_more=int((count >= 2).sum()),
               refused_by_keep=int(refused.sum()), five_or_more=int((count >= 5).sum()), six_or_more=int((count >= 6).sum()))
    return out


def same(got, want):
    """None when every layer and count of got equals want's, else the first that differs"""
    for key in LAYERS:
        if got[key].shape != want[key].shape or got[key].dtype != want[key].dtype or got[key].tobytes() != want[key].tobytes():
            return key
    for key in COUNTS:
        if got[key] != want[key]:
            return key
    return None


def tile(parts, rows, cols):
    """the layers of rows x cols rectangle results (row-major list) put together"""
    return {key: np.concatenate([np.concatenate([parts[r * cols + c][key] for c in range(cols)], axis=1) for r in range(rows)], axis=0)
            for key in LAYERS}
