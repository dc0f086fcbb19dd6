"""numpy restatement of the mask distance maps ("Mask distance maps"), written from the definition and not from
the kernels: brute force of the 64-bit key (d2 << 32) | index over ALL background pixels, for small images only.  Plus the
masks the CPU and GPU suites share."""
import numpy as np

SENTINEL_D2 = 0xFFFFFFFF
# (H, W) of the suites: one pixel, one row, one column, odd sizes, a row wider than one workgroup of 256, a segment of 64 rows
SHAPES = [(1, 1), (1, 70), (70, 1), (45, 70), (33, 129), (64, 64), (3, 257)]
DENSITIES = [0.0, 0.02, 0.5, 0.97, 1.0]  # share of foreground pixels; 1.0 = no background at all


def edt(mask, threshold=0):
    """(d2 uint32, nearest int32) of a (H, W) uint8 mask: foreground iff mask > threshold."""
    mask = np.asarray(mask, np.uint8)
    h, w = mask.shape
    d2 = np.full(h * w, SENTINEL_D2, np.uint32)
    nearest = np.full(h * w, -1, np.int32)
    by, bx = np.nonzero(mask <= threshold)
    if len(by):
        index = by.astype(np.uint64) * np.uint64(w) + bx.astype(np.uint64)
        py, px = np.divmod(np.arange(h * w, dtype=np.int64), w)
        for lo in range(0, h * w, 1024):  # blocks of pixels x all background pixels
            dy = py[lo:lo + 1024, None] - by[None, :]
            dx = px[lo:lo + 1024, None] - bx[None, :]
            key = ((dy * dy + dx * dx).astype(np.uint64) << np.uint64(32)) | index[None, :]
            best = key.min(axis=1)
            d2[lo:lo + 1024] = (best >> np.uint64(32)).astype(np.uint32)
            nearest[lo:lo + 1024] = (best & np.uint64(0xFFFFFFFF)).astype(np.int32)
    return d2.reshape(h, w), nearest.reshape(h, w)


def edt_at(mask, pixels, threshold=0):
    """the same brute force for the given linear pixel indices only (images too large for edt): (d2, nearest) per pixel"""
    mask = np.asarray(mask, np.uint8)
    h, w = mask.shape
    by, bx = np.nonzero(mask <= threshold)
    assert len(by), "edt_at needs a background pixel"
    index = by.astype(np.uint64) * np.uint64(w) + bx.astype(np.uint64)
    pixels = np.asarray(pixels, np.int64)
    d2 = np.empty(len(pixels), np.uint32)
    nearest = np.empty(len(pixels), np.int32)
    py, px = np.divmod(pixels, w)
    for lo in range(0, len(pixels), 64):
        dy = py[lo:lo + 64, None] - by[None, :]
        dx = px[lo:lo + 64, None] - bx[None, :]
        best = (((dy * dy + dx * dx).astype(np.uint64) << np.uint64(32)) | index[None, :]).min(axis=1)
        d2[lo:lo + 64] = (best >> np.uint64(32)).astype(np.uint32)
        nearest[lo:lo + 64] = (best & np.uint64(0xFFFFFFFF)).astype(np.int32)
    return d2, nearest


def random_mask(shape, density, seed):
    """uint8 mask with about `density` of its pixels foreground (values 1..255), the rest 0"""
    rng = np.random.default_rng(seed)
    h, w = shape
    if density >= 1.0:
        return rng.integers(1, 256, (h, w)).astype(np.uint8)
    fg = rng.random((h, w)) < density
    return np.where(fg, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)


def byte_mask(shape, seed):
    """every byte value, for the threshold cases"""
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def tie_mask():
    """5 x 5, all foreground except (0,2), (2,0), (2,4), (4,2): the centre is 2 away from all four, index 2 is the lowest"""
    m = np.full((5, 5), 255, np.uint8)
    for y, x in ((0, 2), (2, 0), (2, 4), (4, 2)):
        m[y, x] = 0
    return m


def crack_mask(shape, seed, cracks=5):
    """thin random-walk cracks 1-7 px wide: FOREGROUND (255) lines on a background of 0, as a segmentation mask has them"""
    rng = np.random.default_rng(seed)
    h, w = shape
    m = np.zeros((h, w), np.uint8)
    for _ in range(cracks):
        y, x = rng.uniform(0, h), rng.uniform(0, w)
        heading = rng.uniform(0, 2 * np.pi)
        half = rng.integers(0, 4)  # width 1, 3, 5 or 7
        for _ in range(int(rng.integers(w // 2, 2 * w))):
            heading += rng.normal(0, 0.25)
            y, x = y + np.sin(heading), x + np.cos(heading)
            iy, ix = int(round(y)), int(round(x))
            if not (0 <= iy < h and 0 <= ix < w):
                break
            if rng.random() < 0.02:
                half = rng.integers(0, 4)
            m[max(0, iy - half):iy + half + 1, max(0, ix - half):ix + half + 1] = 255
    return m


def corner_mask(shape):
    """everything foreground but the far corner: the longest search a pixel can have"""
    m = np.full(shape, 255, np.uint8)
    m[-1, -1] = 0
    return m
