"""Restatement of the crack lengths on the map ("Crack lengths on the map", CL1-CL9), written from the rules and not
from csrc/pcp_crack_length.hpp: the links of _crack_fuse_ref.links, CL2 with math.isqrt on Python integers, the distances by
scipy's Dijkstra on the integer weights (exact in fp64: every sum stays below 2^53, asserted), CL4-CL7 in plain Python.  Plus
the two clouds of known length the CPU and GPU suites share."""
import math

import numpy as np

import _crack_fuse_ref as ref

NO_POS = 2 ** 64 - 1
UNIT = 2.0 ** -20  # metres per unit of length_q and pos
BAND_SEED, ARC_SEED = 3, 7  # (seeds at which 4 000 uniform samples leave no gap of 5 mm: the clouds are one crack each)


def weight(d2):
    """CL2 for one fp32 squared distance: trunc(d2 * 2^40) as a Python integer (the product is exact), its integer root, >= 1"""
    k = int(float(np.float32(d2)) * 2.0 ** 40)
    assert 0 <= k <= 2 ** 40
    return max(1, math.isqrt(k))


def weighted_links(xyz, views, min_views, radius):
    """pairs (k, 2) int64 with i < j, and w (k,) int64"""
    xyz = np.asarray(xyz, np.float32)
    pairs = ref.links(xyz, views, min_views, radius)
    d = xyz[pairs[:, 1]] - xyz[pairs[:, 0]]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == np.float32
    return pairs, np.array([weight(v) for v in d2], np.int64)


def _distances(n, pairs, w, sources):
    """D from each node's own component's source (the components share no edge, so the minimum over the sources is that), int64;
    -1 where no source reaches"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra

    adj = coo_matrix((w.astype(np.float64), (pairs[:, 0], pairs[:, 1])), shape=(n, n)).tocsr()
    d = dijkstra(adj, directed=False, indices=np.asarray(sources, np.int64), min_only=True)
    fin = np.isfinite(d)
    assert (d[fin] < 2.0 ** 53).all() and (d[fin] == np.rint(d[fin])).all()
    return np.where(fin, d, -1.0).astype(np.int64)


def _farthest(label, ids, d):
    """per crack: the lowest index among the maxima of d"""
    out = []
    for c in ids.tolist():
        mem = np.flatnonzero(label == c)
        out.append(int(mem[np.flatnonzero(d[mem] == d[mem].max())[0]]))
    return out


def lengths(xyz, views, min_views, radius, sum_q=None):
    """dict(pos (n,) uint64, ids (C,) int32, rows (C, 7) int64, offsets (C + 1,) int64, path int32, label)"""
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    pairs, w = weighted_links(xyz, views, min_views, radius)
    label = ref.components(xyz, views, min_views, radius, pairs)
    ids = np.unique(label[label >= 0]).astype(np.int32)
    pos = np.full(n, NO_POS, np.uint64)
    rows = np.zeros((len(ids), 7), np.int64)
    offsets = np.zeros(len(ids) + 1, np.int64)
    path = []
    if len(ids):
        d0 = _distances(n, pairs, w, ids)  # CL4: s0 is the label
        a = _farthest(label, ids, d0)
        da = _distances(n, pairs, w, a)
        b = _farthest(label, ids, da)
        who = label >= 0
        assert (da[who] >= 0).all() and (d0[who] >= 0).all()
        pos[who] = da[who].astype(np.uint64)
        nbr = {}
        for (i, j), wij in zip(pairs.tolist(), w.tolist()):
            nbr.setdefault(i, []).append((j, wij))
            nbr.setdefault(j, []).append((i, wij))
        if sum_q is None:
            fw = np.zeros(n, np.int64)
        else:
            fw = ref.fused_w(dict(sum_q=np.asarray(sum_q), views=np.asarray(views)))
        for r in range(len(ids)):
            chain = [b[r]]
            while chain[-1] != a[r]:  # CL6
                i = chain[-1]
                cand = [j for j, wij in nbr[i] if int(da[j]) + wij == int(da[i])]
                assert cand and len(chain) <= n
                chain.append(min(cand))
            chain.reverse()
            f = fw[chain]
            rows[r] = (a[r], b[r], int(da[b[r]]), len(chain) - 1, int(f.sum()), int(f.min()), int(f.max()))
            path.extend(chain)
            offsets[r + 1] = len(path)
    return dict(pos=pos, ids=ids, rows=rows, offsets=offsets, path=np.array(path, np.int32).reshape(-1), label=label)


KEYS = ("pos", "ids", "rows", "offsets", "path")


def assert_same(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype, (what, k, got[k].dtype, want[k].dtype)
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


# ---- clouds of known length -------------------------------------------------------------------------------------------------
def band(n=4000, seed=BAND_SEED):
    """a straight band 2 m x 4 mm in the plane z = 0, uniformly sampled"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.0, 2.0, n), rng.uniform(-0.002, 0.002, n), np.zeros(n)], axis=1).astype(np.float32)


def arc(n=4000, seed=ARC_SEED):
    """a quarter circle of radius 1 m, +-2 mm across, in the plane z = 0"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0.0, np.pi / 2.0, n)
    rad = 1.0 + rng.uniform(-0.002, 0.002, n)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(n)], axis=1).astype(np.float32)
