"""The voxel-grid output restated ("Voxel-grid output", VG1-VG7): numpy for the fp32 cell, Python integers for the
fixed-point positions, the sums and the finish.  Shared by the CPU and the GPU suites; nothing here calls the library."""
import numpy as np

BIAS = 1 << 20
TWO32 = 1 << 32


def cells(leaf, xyz):
    """(n, 3) int64 cells: floorf of the fp32 product with inv = f32(1 / leaf)."""
    inv = np.float32(1.0) / np.float32(leaf)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor(np.asarray(xyz, np.float32) * inv).astype(np.float64).astype(np.int64)


def key_of(c):
    return ((int(c[2]) + BIAS) << 42) | ((int(c[1]) + BIAS) << 21) | (int(c[0]) + BIAS)


def fixed(x):
    """llrint((double)x * 2^32): the product is exact, round() of a Python float rounds half to even."""
    return round(float(x) * 4294967296.0)


def corner(c, leaf):
    return round(float(c) * float(np.float32(leaf)) * 4294967296.0)


def accumulate(leaf, xyz, rgb, label=None, sums=None):
    """Adds the rows into `sums` (a dict key -> [cells, [q0, q1, q2], n, r, g, b, label]) and returns it."""
    sums = {} if sums is None else sums
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    cs = cells(leaf, xyz)
    for i in range(xyz.shape[0]):
        c = cs[i]
        k = key_of(c)
        s = sums.get(k)
        if s is None:
            s = sums[k] = [tuple(int(v) for v in c), [0, 0, 0], 0, 0, 0, 0, 0]
        for a in range(3):
            s[1][a] += fixed(xyz[i, a]) - corner(s[0][a], leaf)
        s[2] += 1
        s[3] += int(rgb[i, 0])
        s[4] += int(rgb[i, 1])
        s[5] += int(rgb[i, 2])
        s[6] += 0 if label is None else int(label[i])
    return sums


def finish(leaf, sums):
    """dict(xyz, rgb, label, count) in ascending key order."""
    keys = sorted(sums)
    m = len(keys)
    xyz = np.empty((m, 3), np.float32)
    rgb = np.empty((m, 3), np.uint8)
    label = np.empty(m, np.uint8)
    count = np.empty(m, np.uint32)
    for j, k in enumerate(keys):
        c, q, n, r, g, b, lab = sums[k]
        for a in range(3):
            fix = corner(c[a], leaf) + (2 * q[a] + n) // (2 * n)  # Python's // floors
            xyz[j, a] = np.float32(float(fix) * 2.0 ** -32)
        rgb[j] = (r // n, g // n, b // n)
        label[j] = lab // n
        count[j] = n
    return dict(xyz=xyz, rgb=rgb, label=label, count=count)


def reduce(leaf, xyz, rgb, label=None):
    return finish(leaf, accumulate(leaf, xyz, rgb, label))


def same(got, want, with_label=False):
    """None, or the name of the first array that differs bit for bit."""
    for k in ("xyz", "rgb", "count") + (("label",) if with_label else ()):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            return k
    return None
