"""Restatement of the crack skeletons on the map ("Crack skeletons on the map", CS1-CS9), written from the rules and
not from csrc/pcp_crack_skeleton.hpp: pos and the links from _crack_length_ref / _crack_fuse_ref, the bands in Python integers,
the nodes by scipy's connected components of the links inside a band (relabelled to the lowest index), the edges by
numpy.unique, CS4, CS6 and CS7 in plain numpy.  Plus the seeded clouds of known topology the CPU and GPU suites share: all in the
plane z = 0, 4 mm across, uniformly sampled."""
import math

import numpy as np

import _crack_fuse_ref as ref
import _crack_length_ref as cl_ref

KEYS = ("node", "ids", "nodes", "edges", "cracks")
METRES = ("centroids", "edge_length_m", "skeleton_length_m")
UNIT = 2.0 ** -20


def step_q_of(step):
    """CS2: trunc((double)step * 2^20) for the fp32 step"""
    return int(float(np.float32(step)) * 2.0 ** 20)


def w_max(radius):
    """the largest weight CL2 gives a link: isqrt(trunc((double)t * 2^40))"""
    return math.isqrt(int(float(ref.threshold_of(radius)) * 2.0 ** 40))


def default_step(radius):
    return float(np.float32(2.0) * np.float32(radius))


def base(xyz, views, min_views, radius, sum_q=None):
    """what does not depend on the step: CS1's pos, labels and links, computed once per cloud"""
    xyz = np.asarray(xyz, np.float32)
    return dict(lengths=cl_ref.lengths(xyz, views, min_views, radius, sum_q), pairs=ref.links(xyz, views, min_views, radius))


def skeleton(xyz, views, min_views, radius, step, sum_q=None, base_of=None):
    """dict(node (n,) int32, ids (N,) int32, nodes (N, 10) int64, edges (E, 3) int64, cracks (C, 6) int64, centroids (N, 3),
    edge_length_m (E,), skeleton_length_m (C,), plus band (n,) int64 (-1: no crack point), pairs, label, pos)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    if base_of is None:
        base_of = base(xyz, views, min_views, radius, sum_q)
    pos, label, crack_ids, pairs = base_of["lengths"]["pos"], base_of["lengths"]["label"], base_of["lengths"]["ids"], base_of["pairs"]
    sq = step_q_of(step)
    assert sq >= w_max(radius) and float(np.float32(step)) <= 16.0
    who = np.flatnonzero(label >= 0)
    band = np.full(n, -1, np.int64)
    band[who] = [int(pos[i]) // sq for i in who.tolist()]  # CS2, Python integers
    same = band[pairs[:, 0]] == band[pairs[:, 1]]
    inner = pairs[same]
    adj = coo_matrix((np.ones(len(inner), np.int8), (inner[:, 0], inner[:, 1])), shape=(n, n))
    _, comp = connected_components(adj, directed=False)
    lowest = np.full(n, n, np.int64)
    np.minimum.at(lowest, comp[who], who)
    node = np.full(n, -1, np.int32)
    node[who] = lowest[comp[who]]  # CS3
    ids = np.unique(node[who]).astype(np.int32)
    row = np.full(n, -1, np.int64)
    row[who] = np.searchsorted(ids, node[who])
    # CS4
    nodes = np.zeros((len(ids), 10), np.int64)
    nodes[:, 0] = np.searchsorted(crack_ids, label[ids])
    nodes[:, 1] = band[ids]
    fw = ref.fused_w(dict(sum_q=np.asarray(sum_q), views=np.asarray(views))) if sum_q is not None else np.zeros(n, np.int64)
    np.add.at(nodes[:, 2], row[who], 1)
    np.add.at(nodes[:, 3], row[who], fw[who])
    nodes[:, 4] = np.iinfo(np.int64).max
    np.minimum.at(nodes[:, 4], row[who], fw[who])
    np.maximum.at(nodes[:, 5], row[who], fw[who])
    with np.errstate(invalid="ignore"):
        q = np.floor(xyz[who].astype(np.float64) * 2.0 ** 20).astype(np.int64)  # (crack points are finite)
    assert (np.abs(xyz[who]) <= 2.0 ** 20).all()
    for a in range(3):
        np.add.at(nodes[:, 6 + a], row[who], q[:, a])
    # CS5
    cross = pairs[~same]
    low_first = band[cross[:, 0]] < band[cross[:, 1]]
    u = row[np.where(low_first, cross[:, 0], cross[:, 1])]
    v = row[np.where(low_first, cross[:, 1], cross[:, 0])]
    if len(cross):
        uv, links = np.unique(np.stack([u, v], axis=1), axis=0, return_counts=True)
        edges = np.concatenate([uv, links[:, None]], axis=1).astype(np.int64)
    else:
        edges = np.zeros((0, 3), np.int64)
    nodes[:, 9] = np.bincount(edges[:, 0], minlength=len(ids)) + np.bincount(edges[:, 1], minlength=len(ids))
    # CS6
    c = len(crack_ids)
    cracks = np.zeros((c, 6), np.int64)
    cracks[:, 0] = np.bincount(nodes[:, 0], minlength=c)
    cracks[:, 1] = np.bincount(nodes[edges[:, 0], 0], minlength=c)
    cracks[:, 2] = np.bincount(nodes[nodes[:, 9] == 1, 0], minlength=c)
    cracks[:, 3] = np.bincount(nodes[nodes[:, 9] >= 3, 0], minlength=c)
    cracks[:, 4] = cracks[:, 1] - cracks[:, 0] + 1
    np.maximum.at(cracks[:, 5], nodes[:, 0], nodes[:, 9])
    out = dict(node=node, ids=ids, nodes=nodes, edges=edges, cracks=cracks, band=band, pairs=pairs, label=label, pos=pos)
    out.update(metres(nodes, edges, c))
    return out


def metres(nodes, edges, cracks):
    """CS7 in fp64: centroids, the edges' lengths, and per crack their sum in row order (one addition after the other)"""
    centroids = (nodes[:, 6:9].astype(np.float64) / nodes[:, 2:3].astype(np.float64)) * UNIT
    d = centroids[edges[:, 1]] - centroids[edges[:, 0]]
    edge_length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    length = [0.0] * cracks
    for r, e in zip(nodes[edges[:, 0], 0].tolist(), edge_length.tolist()):
        length[r] += e
    return dict(centroids=centroids, edge_length_m=edge_length, skeleton_length_m=np.array(length, np.float64).reshape(-1))


def assert_same(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype, (what, k, got[k].dtype, want[k].dtype)
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def check_rules(want, what=""):
    """what CS2-CS6 promise, on the restatement alone, for every crack"""
    band, pairs, label, pos, node = want["band"], want["pairs"], want["label"], want["pos"], want["node"]
    nodes, edges, cracks, ids = want["nodes"], want["edges"], want["cracks"], want["ids"]
    assert (np.abs(band[pairs[:, 0]] - band[pairs[:, 1]]) <= 1).all(), (what, "linked points are at most one band apart")
    assert np.array_equal(node >= 0, label >= 0) and np.array_equal(node[ids], ids), what
    assert (nodes[edges[:, 1], 1] - nodes[edges[:, 0], 1] == 1).all(), (what, "an edge joins adjacent bands, u the lower")
    assert (nodes[edges[:, 0], 0] == nodes[edges[:, 1], 0]).all() and (edges[:, 2] >= 1).all(), what
    if len(edges) > 1:
        key = edges[:, 0] * (len(ids) + 1) + edges[:, 1]
        assert (np.diff(key) > 0).all(), (what, "edges unique and ascending")
    assert edges[:, 2].sum() == (band[pairs[:, 0]] != band[pairs[:, 1]]).sum(), (what, "every cross-band link is counted once")
    crack_ids = np.unique(label[label >= 0])
    assert len(cracks) == len(crack_ids)
    for r, c in enumerate(crack_ids.tolist()):
        mine = np.flatnonzero(nodes[:, 0] == r)
        zero = mine[nodes[mine, 1] == 0]
        end_a = int(np.flatnonzero((label == c) & (pos == 0))[0])
        assert len(zero) == 1 and node[end_a] == ids[zero[0]], (what, r, "exactly one band-0 node, and it holds end_a")
        assert nodes[mine, 2].sum() == (label == c).sum(), (what, r, "the node points add up to the crack's points")
        assert cracks[r, 4] >= 0 and cracks[r, 0] == len(mine), (what, r)
        if len(mine) == 1:
            assert cracks[r].tolist() == [1, 0, 0, 0, 0, 0], (what, r)


# ---- clouds of known topology -------------------------------------------------------------------------------------------------
def _arms(angles_deg, length, per_arm, seed):
    """arms from the origin, each `length` long and 4 mm across, per_arm uniform samples each"""
    rng = np.random.default_rng(seed)
    out = []
    for deg in angles_deg:
        a = np.radians(deg)
        along, across = rng.uniform(0.0, length, per_arm), rng.uniform(-0.002, 0.002, per_arm)
        out.append(np.stack([along * np.cos(a) - across * np.sin(a), along * np.sin(a) + across * np.cos(a), np.zeros(per_arm)], axis=1))
    return np.concatenate(out).astype(np.float32)


def y_cloud(seed, length=0.6, per_arm=1300):
    return _arms((90.0, 210.0, 330.0), length, per_arm, seed)


def small_y(seed):
    return y_cloud(seed, 0.12, 300)


def plus_cloud(seed, length=0.6, per_arm=1300):
    return _arms((0.0, 90.0, 180.0, 270.0), length, per_arm, seed)


def ring_cloud(seed, n=4000, radius=0.3):
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    rad = radius + rng.uniform(-0.002, 0.002, n)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(n)], axis=1).astype(np.float32)


def wall_cloud(seed=1, n=4000):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.0, 0.12, n), rng.uniform(0.0, 0.08, n), np.zeros(n)], axis=1).astype(np.float32)


def shape_cases():
    """name -> xyz of the shapes whose topology the suites assert (views 1, min_views 1)"""
    out = {"band": cl_ref.band(), "arc": cl_ref.arc(), "wall": wall_cloud(1)}
    for s in (1, 2, 3, 4):
        out[f"y{s}"] = y_cloud(s)
    for s in (1, 2, 4):
        out[f"plus{s}"] = plus_cloud(s)
    for s in (1, 2, 3):
        out[f"ring{s}"] = ring_cloud(s)
        out[f"small_y{s}"] = small_y(s)
    return out
