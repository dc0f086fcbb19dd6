"""A numpy restatement of the keyframe colour balance ("Image balance", IB1-IB9), written from the rules and
independent of the C++: a materialised reflected pad, np.bincount per tile, a Python loop for the residual walk, fp32 arrays
with one operation per statement.  The two HSV halves are restated here the way oracle/np_oracle.py's hsv_round_trip writes
them (the oracle exposes only the whole round trip); hsv_halves_agree_with_the_oracle() ties them to it.

Also the shapes, images and parameters the image balance tests share."""
import numpy as np

f32 = np.float32

# (w, h, tiles_x, tiles_y): see each line
SHAPES = [
    (64, 48, 8, 8),     # divides evenly; 48-pixel tiles, so clip falls to its floor of 1
    (70, 50, 8, 8),     # both sides padded, to 72 x 56
    (64, 50, 8, 8),     # only the height fails to divide: the width is extended by a whole 8
    (48, 36, 1, 1),     # a single tile: both interpolation indices clamp to it
    (90, 60, 3, 5),
    (128, 128, 16, 16),
    (512, 384, 2, 2),   # 49 152-pixel tiles: several workgroups per tile, the global merge
]
IMAGES = ["noise", "ramp", "constant", "two_level", "blob"]
CLIPS = [0.0, 1.0, 3.0, 40.0]
GAMMAS = [0.8, 1.0, 1.1]
STAGES = [1, 2, 3]


def image(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 + seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":  # horizontal ramp with a colour cast
        v = (np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)
        im = np.empty((h, w, 3), np.uint8)
        im[..., 0] = v // 2
        im[..., 1] = v
        im[..., 2] = (v.astype(np.int32) * 3 // 4).astype(np.uint8)
        return im
    if kind == "constant":  # every pixel in one bin: the residual walk with step > 1
        im = np.empty((h, w, 3), np.uint8)
        im[...] = (40, 97, 60)
        return im
    if kind == "two_level":  # V only 0 and 255
        on = rng.random((h, w)) < 0.3
        im = np.zeros((h, w, 3), np.uint8)
        im[on] = (255, 30, 200)
        return im
    if kind == "blob":  # dark, with one saturated blob
        im = rng.integers(0, 30, (h, w, 3), dtype=np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        im[(yy - h // 3) ** 2 + (xx - 2 * w // 3) ** 2 <= (min(w, h) // 6) ** 2] = (255, 255, 255)
        return im
    raise ValueError(kind)


def looks_real(w: int, h: int) -> np.ndarray:
    """ramp + blob + a little noise: what a tunnel keyframe roughly looks like"""
    rng = np.random.default_rng(7)
    base = image("ramp", w, h).astype(np.int32) // 2 + rng.integers(0, 12, (h, w, 3))
    yy, xx = np.mgrid[0:h, 0:w]
    base[(yy - h // 3) ** 2 + (xx - 2 * w // 3) ** 2 <= (min(w, h) // 8) ** 2] = 255
    return np.clip(base, 0, 255).astype(np.uint8)


# ---- the HSV halves (OpenCV 4.2 RGB2HSV_b / HSV2RGB_native, as np_oracle.hsv_round_trip restates the whole) ----------------
def _sat(x):
    return np.clip(np.rint(np.asarray(x, f32)).astype(np.int64), 0, 255)


def hsv_forward(bgr):
    a = np.asarray(bgr, np.uint8).reshape(-1, 3).astype(np.int64)
    b, g, r = a[:, 0], a[:, 1], a[:, 2]
    idx = np.arange(1, 256, dtype=np.float64)
    sdiv = np.concatenate([[0], np.rint((255 << 12) / (1.0 * idx)).astype(np.int64)])
    hdiv = np.concatenate([[0], np.rint((180 << 12) / (6.0 * idx)).astype(np.int64)])
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * sdiv[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.clip(h, 0, 255), s & 0xFF, v


def hsv_backward(H, S, V):
    inv255 = f32(1.0) / f32(255.0)
    fs = S.astype(f32) * inv255
    fv = V.astype(f32) * inv255
    fh = H.astype(f32) * (f32(6.0) / f32(180.0))
    fh = np.fmod(fh, f32(6.0)).astype(f32)
    sector = np.floor(fh).astype(np.int64)
    fh = fh - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    fh = np.where(bad, f32(0), fh).astype(f32)
    one = f32(1.0)
    t1 = one - fs
    t1 = fv * t1
    t2 = fs * fh
    t2 = one - t2
    t2 = fv * t2
    t3 = one - fh
    t3 = fs * t3
    t3 = one - t3
    t3 = fv * t3
    tab = np.stack([fv, t1, t2, t3], axis=1).astype(f32)
    sector_data = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    pick = sector_data[sector]
    rows = np.arange(len(tab))
    out = np.stack([tab[rows, pick[:, c]] for c in range(3)], axis=1)
    grey = fs == 0
    out[grey] = fv[grey, None]
    return _sat(out * f32(255.0)).astype(np.uint8)


def hsv_halves_agree_with_the_oracle(bgr) -> bool:
    from oracle import np_oracle

    H, S, V = hsv_forward(bgr)
    mine = hsv_backward(H, S, V).reshape(np.asarray(bgr).shape)
    return np.array_equal(mine, np_oracle.hsv_round_trip(bgr, 1.0, 1.0))


# ---- IB3-IB8 -------------------------------------------------------------------------------------------------------------
def grid(w, h, tiles_x, tiles_y):
    """(ext_x, ext_y, tw, th) or None when a reflected index would leave the image"""
    ext_x = ext_y = 0
    if w % tiles_x != 0 or h % tiles_y != 0:
        ext_x = tiles_x - w % tiles_x
        ext_y = tiles_y - h % tiles_y
    if ext_x >= w or ext_y >= h:
        return None
    return ext_x, ext_y, (w + ext_x) // tiles_x, (h + ext_y) // tiles_y


def gamma_table(gamma) -> np.ndarray:
    inv = 1.0 / float(f32(gamma))  # the C ABI carries gamma as a float
    return np.array([((i / 255.0) ** inv) * 255.0 for i in range(256)]).astype(np.uint8)


def clahe_tables(V, tiles_x, tiles_y, clip_limit):
    """V (h, w) int -> (hist (ty, tx, 256) uint32, lut (ty, tx, 256) uint8)"""
    h, w = V.shape
    ext_x, ext_y, tw, th = grid(w, h, tiles_x, tiles_y)
    padded = np.pad(V, ((0, ext_y), (0, ext_x)), mode="reflect")
    total = tw * th
    hist = np.zeros((tiles_y, tiles_x, 256), np.uint32)
    lut = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    clip = 0
    if f32(clip_limit) > 0:
        clip = max(int(float(f32(clip_limit)) * total / 256), 1)
    lut_scale = f32(255.0) / f32(total)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile = padded[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            hh = np.bincount(tile.ravel(), minlength=256).astype(np.int64)
            hist[ty, tx] = hh
            if clip > 0:
                clipped = int(np.maximum(hh - clip, 0).sum())
                hh = np.minimum(hh, clip)
                batch = clipped // 256
                hh = hh + batch
                residual = clipped - 256 * batch
                if residual != 0:
                    step = max(256 // residual, 1)
                    i = 0
                    while i < 256 and residual > 0:
                        hh[i] += 1
                        i += step
                        residual -= 1
            cum = np.cumsum(hh).astype(f32)
            scaled = cum * lut_scale
            lut[ty, tx] = _sat(scaled)
    return hist, lut


def _weights(n, size, tiles):
    inv = f32(1.0) / f32(size)
    t = np.arange(n).astype(f32)
    t = t * inv
    t = t - f32(0.5)
    fl = np.floor(t)
    a = (t - fl).astype(f32)
    a1 = (f32(1.0) - a).astype(f32)
    t1 = fl.astype(np.int64)
    t2 = t1 + 1
    return np.maximum(t1, 0), np.minimum(t2, tiles - 1), a, a1


def clahe_apply(V, lut, tiles_x, tiles_y):
    h, w = V.shape
    _, _, tw, th = grid(w, h, tiles_x, tiles_y)
    x1, x2, xa, xa1 = _weights(w, tw, tiles_x)
    y1, y2, ya, ya1 = _weights(h, th, tiles_y)
    Y1, Y2 = y1[:, None], y2[:, None]
    X1, X2 = x1[None, :], x2[None, :]
    l11 = lut[Y1, X1, V].astype(f32)
    l12 = lut[Y1, X2, V].astype(f32)
    l21 = lut[Y2, X1, V].astype(f32)
    l22 = lut[Y2, X2, V].astype(f32)
    p = l11 * xa1[None, :]
    q = l12 * xa[None, :]
    top = (p + q).astype(f32)
    p = l21 * xa1[None, :]
    q = l22 * xa[None, :]
    bottom = (p + q).astype(f32)
    p = top * ya1[:, None]
    q = bottom * ya[:, None]
    return _sat((p + q).astype(f32))


def balance(bgr, stages=3, tiles=(8, 8), clip_limit=1.0, gamma=0.8) -> dict:
    """dict(bgr, hist, lut) (hist, lut None without the CLAHE stage)"""
    bgr = np.asarray(bgr, np.uint8)
    h, w = bgr.shape[:2]
    out = bgr.copy()
    hist = lut = None
    if stages & 1:
        H, S, V = hsv_forward(bgr)
        Vim = V.reshape(h, w)
        hist, lut = clahe_tables(Vim, tiles[0], tiles[1], clip_limit)
        V2 = clahe_apply(Vim, lut, tiles[0], tiles[1]).reshape(-1)
        out = hsv_backward(H, S, V2).reshape(h, w, 3)
    if stages & 2:
        out = gamma_table(gamma)[out]
    return dict(bgr=out, hist=hist, lut=lut)
