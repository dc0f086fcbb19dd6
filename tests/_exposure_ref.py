"""Restatement of the exposure-gain rules EG1-EG5 ("Exposure gains") in numpy: what the GPU statistics, the
library's solve and the gained finalise are compared against.  Inputs are top-5 lists in the form pcp_colour_finalise and
the oracle report them: (n, 5) arrays, top_frame -1 in the empty slots, top_rgb 0x00RRGGBB."""
import numpy as np

# the property scene: keyframe f of small_scene is a uniform grey of round(128 k_f)
K_EXPOSURE = (0.6, 1.4, 0.8, 1.2, 1.0, 0.7)


def grey_images(cd):
    return [np.full((cd["image_height"], cd["image_width"], 3), int(round(128 * k)), np.uint8) for k in K_EXPOSURE]


def equalisation_ratio(g):
    """spread of log(g_f k_f) over the spread of log(k_f)"""
    k = np.asarray(K_EXPOSURE)
    return float(np.std(np.log(np.asarray(g) * k)) / np.std(np.log(k)))


def luma(top_rgb):
    """EG1: integer luma of the colour words (the top byte is masked)."""
    c = np.asarray(top_rgb).astype(np.int64) & 0xFFFFFF
    return (77 * ((c >> 16) & 0xFF) + 150 * ((c >> 8) & 0xFF) + 29 * (c & 0xFF) + 128) >> 8


def usable(top_frame, top_rgb):
    """EG2: listed and not clipped."""
    y = luma(top_rgb)
    return (np.asarray(top_frame) >= 0) & (y >= 8) & (y <= 247)


def pair_stats(top_frame, top_rgb, F):
    """EG3: (n, sum), uint64 (F, F) each."""
    tf = np.asarray(top_frame).astype(np.int64)
    y = luma(top_rgb)
    ok = usable(tf, top_rgb)
    n = np.zeros((F, F), np.uint64)
    s = np.zeros((F, F), np.uint64)
    for a in range(5):
        for b in range(5):
            if a == b:
                continue
            m = ok[:, a] & ok[:, b] & (tf[:, a] != tf[:, b])
            np.add.at(n, (tf[m, a], tf[m, b]), np.uint64(1))
            np.add.at(s, (tf[m, a], tf[m, b]), y[m, a].astype(np.uint64))
    return n, s


def excluded_pairs(top_frame, top_rgb):
    """Ordered pairs of listed views from two keyframes that EG2 keeps out of the statistics."""
    tf = np.asarray(top_frame).astype(np.int64)
    ok = usable(tf, top_rgb)
    count = 0
    for a in range(5):
        for b in range(5):
            if a != b:
                listed = (tf[:, a] >= 0) & (tf[:, b] >= 0) & (tf[:, a] != tf[:, b])
                count += int((listed & ~(ok[:, a] & ok[:, b])).sum())
    return count


def system(n, s, sigma_n=10.0, sigma_g=0.1):
    """EG4: (active keyframes, A, b) of the normal equations."""
    n = np.asarray(n).astype(np.float64)
    s = np.asarray(s).astype(np.float64)
    F = n.shape[0]
    off = n.copy()
    np.fill_diagonal(off, 0.0)
    active = np.nonzero(off.sum(axis=1) > 0)[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(off > 0, s / n, 0.0)  # I_ij
    A = np.zeros((F, F))
    b = np.zeros(F)
    for i in active:
        for j in active:
            if i == j or off[i, j] == 0:
                continue
            A[i, i] += off[i, j] * (mean[i, j] ** 2 / sigma_n**2 + 1.0 / sigma_g**2)
            A[i, j] -= off[i, j] * mean[i, j] * mean[j, i] / sigma_n**2
            b[i] += off[i, j] / sigma_g**2
    return active, A[np.ix_(active, active)], b[active]


def gains(n, s, sigma_n=10.0, sigma_g=0.1):
    """EG4: one gain per keyframe; 1.0 exactly for a keyframe without a pair."""
    g = np.ones(np.asarray(n).shape[0], np.float64)
    active, A, b = system(n, s, sigma_n, sigma_g)
    if len(active):
        g[active] = np.linalg.solve(A, b)
    return g


def gained_channel(c, g32):
    """EG5: a channel (array of 0..255) under fp32 gains of the same shape."""
    v = c.astype(np.float32) * g32
    v = v + np.float32(0.5)
    return np.minimum(v.astype(np.int32), 255)


def finalise(top_score, top_rgb, top_frame, gains_per_frame):
    """EG5: (rgb (n, 3) uint8, has (n,) uint8) -- Top5::finalise's fp32 arithmetic over the gained channels."""
    ts = np.asarray(top_score, np.float32)
    tf = np.asarray(top_frame).astype(np.int64)
    c = np.asarray(top_rgb).astype(np.int64) & 0xFFFFFF
    g32 = np.asarray(gains_per_frame, np.float64).astype(np.float32)
    listed = tf >= 0
    gk = np.where(listed, g32[np.where(listed, tf, 0)], np.float32(1.0)).astype(np.float32)
    n = ts.shape[0]
    total = np.zeros(n, np.float32)
    acc = [np.zeros(n, np.float32) for _ in range(3)]
    for k in range(5):
        m = listed[:, k]
        s = np.where(m, ts[:, k], np.float32(0.0)).astype(np.float32)
        for ch, sh in enumerate((16, 8, 0)):
            cg = gained_channel((c[:, k] >> sh) & 0xFF, gk[:, k]).astype(np.float32)
            acc[ch] = np.where(m, acc[ch] + cg * s, acc[ch]).astype(np.float32)
        total = np.where(m, total + s, total).astype(np.float32)
    seen = listed[:, 0]
    rgb = np.zeros((n, 3), np.uint8)
    with np.errstate(invalid="ignore", divide="ignore"):
        for ch in range(3):
            q = np.where(seen, acc[ch] / np.where(seen, total, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
            rgb[:, ch] = (q.astype(np.int64) & 0xFF).astype(np.uint8)
    has = (rgb.any(axis=1) & seen).astype(np.uint8)
    return rgb, has
