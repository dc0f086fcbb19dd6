"""Restatement of the crack branches on the map ("Crack branches on the map", CB1-CB8), written from the rules and not
from csrc/pcp_crack_branch.hpp: the diagram of _crack_skeleton_ref.skeleton, CB2 by scipy's connected components of the
non-junction subgraph (relabelled to the lowest node row), CB3, CB5 and CB7 in Python integers, CB6 by the int64 moments of
_crack_direction_ref restricted to the links inside a branch, CB8 in plain numpy.  Plus two seeded clouds in the style of
_crack_skeleton_ref._arms: a stem with a side twig, and the same with the twig's tip the crack's end b."""
import numpy as np

import _crack_direction_ref as cd_ref
import _crack_fuse_ref as ref
import _crack_skeleton_ref as cs_ref

KEYS = ("branch", "ids", "rows", "moments", "edge_branch", "cracks")
METRES = ("length_m", "kept_length_m", "centroid", "mean_width")
NO_POINT, JUNCTION, PRUNED = -1, -2, -3
BRIDGE, EDGE_PRUNED = -1, -2


def prune_q_of(prune):
    """CB1: trunc((double)prune * 2^20) for the fp32 prune"""
    return int(float(np.float32(prune)) * 2.0 ** 20)


def decompose(n_nodes, edges, keep):
    """CB2 on the node set keep (bool, N): (deg_K (N,), of (N,): the lowest node row of the node's branch, JUNCTION, or PRUNED
    outside K)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    inside = edges[keep[edges[:, 0]] & keep[edges[:, 1]]]
    deg = np.bincount(inside[:, 0], minlength=n_nodes) + np.bincount(inside[:, 1], minlength=n_nodes)
    plain = keep & (deg < 3)
    path = inside[plain[inside[:, 0]] & plain[inside[:, 1]]]
    adj = coo_matrix((np.ones(len(path), np.int8), (path[:, 0], path[:, 1])), shape=(n_nodes, n_nodes))
    _, comp = connected_components(adj, directed=False)
    who = np.flatnonzero(plain)
    lowest = np.full(n_nodes, n_nodes, np.int64)
    np.minimum.at(lowest, comp[who], who)
    of = np.full(n_nodes, PRUNED, np.int64)
    of[keep] = JUNCTION
    of[who] = lowest[comp[who]]
    return deg, of


def branches(xyz, views, min_views, radius, step, prune, sum_q=None, base_of=None, sk=None):
    """dict(branch (n,) int32, ids (B,) int32, rows (B, 15) int64, moments (B, 20) int64, edge_branch (E,) int32, cracks (C, 7)
    int64, length_m (B,), kept_length_m (C,), centroid (B, 3), mean_width (B,), plus node_branch (N,), spur_heads, skeleton)"""
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    if base_of is None:
        base_of = cs_ref.base(xyz, views, min_views, radius, sum_q)
    if sk is None:
        sk = cs_ref.skeleton(xyz, views, min_views, radius, step, sum_q, base_of)
    lengths = base_of["lengths"]
    node, ids, nodes, cracks_cs = sk["node"], sk["ids"], sk["nodes"], sk["cracks"]
    edges = sk["edges"][:, :2]
    N, C = len(ids), len(cracks_cs)
    sq, pq = cs_ref.step_q_of(step), prune_q_of(prune)
    assert 0 <= float(np.float32(prune)) <= 1024.0
    row_of = np.full(n, -1, np.int64)
    who = np.flatnonzero(node >= 0)
    row_of[who] = np.searchsorted(ids, node[who])
    end_nodes = row_of[lengths["rows"][:, :2]].reshape(-1)  # CL7: node[end_a], node[end_b]
    # CB3: the whole diagram, one round
    everything = np.ones(N, bool)
    _, of = decompose(N, edges, everything)
    keep = everything.copy()
    cracks = np.zeros((C, 7), np.int64)
    spur_heads = []
    for h in np.unique(of[of >= 0]).tolist():
        mine = np.flatnonzero(of == h)
        touching = edges[(of[edges[:, 0]] == h) | (of[edges[:, 1]] == h)]
        attachments = int(((of[touching[:, 0]] == JUNCTION) | (of[touching[:, 1]] == JUNCTION)).sum())
        if attachments == 1 and len(mine) * sq < pq and not np.isin(end_nodes, mine).any():
            keep[mine] = False
            spur_heads.append(h)
            r = int(nodes[h, 0])
            cracks[r, 4] += 1
            cracks[r, 5] += len(mine)
            cracks[r, 6] += int(nodes[mine, 2].sum())
    # the final branches
    deg, of = decompose(N, edges, keep)
    heads = np.unique(of[of >= 0])
    B = len(heads)
    node_branch = np.where(of >= 0, np.searchsorted(heads, np.maximum(of, 0)), of).astype(np.int64)
    rows = np.zeros((B, 15), np.int64)
    rows[:, 0] = nodes[heads, 0]
    rows[:, 1] = np.bincount(node_branch[node_branch >= 0], minlength=B)
    rows[:, 4:6] = -1
    edge_branch = np.full(len(edges), EDGE_PRUNED, np.int32)
    for e, (u, v) in enumerate(edges.tolist()):
        if not (keep[u] and keep[v]):
            continue
        bu, bv = int(node_branch[u]), int(node_branch[v])
        if bu == JUNCTION and bv == JUNCTION:
            edge_branch[e] = BRIDGE
            cracks[nodes[u, 0], 1] += 1
        elif bu >= 0 and bv >= 0:
            assert bu == bv
            edge_branch[e] = bu
            rows[bu, 2] += 1
        else:
            b, j = (bu, v) if bu >= 0 else (bv, u)
            edge_branch[e] = b
            rows[b, 3] += 1
            both = sorted(x for x in (int(rows[b, 4]), int(rows[b, 5]), j) if x >= 0)
            rows[b, 4], rows[b, 5] = both[0], (both[1] if len(both) > 1 else -1)
    cracks[:, 0] = np.bincount(rows[:, 0], minlength=C)
    cracks[:, 2] = np.bincount(nodes[keep & (of == JUNCTION), 0], minlength=C)
    cracks[:, 3] = np.bincount(nodes[keep & (deg == 1), 0], minlength=C)
    # CB4, CB5
    brow = np.full(n, NO_POINT, np.int64)
    brow[who] = node_branch[row_of[who]]
    ids_b = ids[heads].astype(np.int32)
    branch = np.where(brow >= 0, ids_b[np.maximum(brow, 0)] if B else 0, brow).astype(np.int32)
    inb = np.flatnonzero(brow >= 0)
    fw = ref.fused_w(dict(sum_q=np.asarray(sum_q), views=np.asarray(views))) if sum_q is not None else np.zeros(n, np.int64)
    pos = lengths["pos"]
    q = np.floor(xyz[inb].astype(np.float64) * 2.0 ** 20).astype(np.int64)
    big = np.iinfo(np.int64).max
    rows[:, 8], rows[:, 10] = big, big
    for k, i in enumerate(inb.tolist()):
        b = int(brow[i])
        w, p = int(fw[i]), int(pos[i])
        rows[b, 6] += 1
        rows[b, 7] += w
        rows[b, 8], rows[b, 9] = min(int(rows[b, 8]), w), max(int(rows[b, 9]), w)
        rows[b, 10], rows[b, 11] = min(int(rows[b, 10]), p), max(int(rows[b, 11]), p)
        rows[b, 12:15] += q[k]
    # CB6: the ordered links whose two points lie in the same final branch
    pairs = sk["pairs"]
    same = pairs[(brow[pairs[:, 0]] >= 0) & (brow[pairs[:, 0]] == brow[pairs[:, 1]])]
    i = np.concatenate([same[:, 0], same[:, 1]])
    j = np.concatenate([same[:, 1], same[:, 0]])
    d = xyz[j] - xyz[i]
    assert d.dtype == np.float32
    dq = np.rint(d * cd_ref.QUANTA).astype(np.int64)
    words = np.zeros((len(i), 10), np.int64)
    words[:, 0] = 1
    words[:, 1:4] = dq
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        words[:, 4 + k] = dq[:, a] * dq[:, b]
    per_point = np.zeros((n, 10), np.int64)
    np.add.at(per_point, i, words)
    sums = [[[0, 0] for _ in range(10)] for _ in range(B)]
    for p in inb.tolist():
        acc = sums[int(brow[p])]
        for k, v_ in enumerate(per_point[p].tolist()):
            lo, hi = cd_ref.split(v_)
            acc[k][0] += lo
            acc[k][1] += hi
    moments = np.array([[h for w in r for h in w] for r in sums], np.int64).reshape(B, 20)
    out = dict(branch=branch, ids=ids_b, rows=rows, moments=moments, edge_branch=edge_branch, cracks=cracks, node_branch=node_branch,
               spur_heads=np.array(spur_heads, np.int64), skeleton=sk, lengths=lengths)
    out.update(metres(rows, edge_branch, nodes, sk["edges"], sk["edge_length_m"], C))
    return out


def metres(rows, edge_branch, nodes, edges, edge_length, cracks):
    """CB8 in fp64: the sums in edge-row order, one addition after the other"""
    length, kept = [0.0] * len(rows), [0.0] * cracks
    for b, r, l in zip(edge_branch.tolist(), nodes[edges[:, 0], 0].tolist(), edge_length.tolist()):
        if b >= 0:
            length[b] += l
        if b >= BRIDGE:
            kept[r] += l
    points = rows[:, 6:7].astype(np.float64)
    return dict(length_m=np.array(length, np.float64).reshape(-1), kept_length_m=np.array(kept, np.float64).reshape(-1),
                centroid=(rows[:, 12:15].astype(np.float64) / points) * cs_ref.UNIT,
                mean_width=(rows[:, 7].astype(np.float64) / points[:, 0]) * cs_ref.UNIT)


def assert_same(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype, (what, k, got[k].dtype, want[k].dtype)
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    for k in METRES:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def check_rules(want, prune, what=""):
    """what CB3, CB6 and CB7 promise, on the restatement alone, for every crack"""
    sk, lengths = want["skeleton"], want["lengths"]
    rows, cracks, node_branch, branch = want["rows"], want["cracks"], want["node_branch"], want["branch"]
    nodes, label = sk["nodes"], sk["label"]
    s1 = want["moments"][:, 2:8].astype(object)
    assert not (s1[:, 1::2] * 2 ** 32 + s1[:, 0::2]).any(), (what, "S1 sums")  # CB6
    assert np.array_equal(branch >= 0, np.isin(branch, want["ids"])) and np.array_equal(branch == NO_POINT, label < 0), what
    if len(want["ids"]):
        assert np.array_equal(branch[want["ids"]], want["ids"]) and (np.diff(want["ids"]) > 0).all(), (what, "ids")
    crack_ids = np.unique(label[label >= 0])
    row_of = np.full(len(label), -1, np.int64)
    who = np.flatnonzero(sk["node"] >= 0)
    row_of[who] = np.searchsorted(sk["ids"], sk["node"][who])
    for r, c in enumerate(crack_ids.tolist()):
        mine = np.flatnonzero(nodes[:, 0] == r)
        b = np.flatnonzero(rows[:, 0] == r)
        kept_j = mine[node_branch[mine] == JUNCTION]
        # CB7's two sums
        assert rows[b, 1].sum() + len(kept_j) + cracks[r, 5] == sk["cracks"][r, 0] == len(mine), (what, r, "nodes")
        assert rows[b, 6].sum() + nodes[kept_j, 2].sum() + cracks[r, 6] == (label == c).sum(), (what, r, "points")
        assert cracks[r, 0] == len(b) >= 1 and cracks[r, 2] == len(kept_j), (what, r)
        assert cracks[r, 5] == (node_branch[mine] == PRUNED).sum() and (cracks[r, 5] > 0) == (cracks[r, 4] > 0), (what, r)
        # CB3's consequence: every node of CL6's path is kept
        path = lengths["path"][lengths["offsets"][r]:lengths["offsets"][r + 1]]
        assert (node_branch[row_of[path]] != PRUNED).all(), (what, r, "the stem is never pruned")
        if len(mine) == 1:
            assert rows[b[0], 1:6].tolist() == [1, 0, 0, -1, -1] and cracks[r].tolist() == [1, 0, 0, 0, 0, 0, 0], (what, r)
    if prune == 0:
        assert not cracks[:, 4:].any() and (node_branch != PRUNED).all() and (want["edge_branch"] != EDGE_PRUNED).all(), (what, "prune 0")
    closed = rows[:, 3] == 0
    assert ((rows[closed, 2] == rows[closed, 1] - 1) | (rows[closed, 2] == rows[closed, 1])).all(), (what, "a path or a cycle")
    assert (rows[~closed, 2] == rows[~closed, 1] - 1).all() and (rows[:, 3] <= 2).all(), (what, "an attached branch is a path")
    assert ((rows[:, 4] >= 0) == (rows[:, 3] >= 1)).all() and ((rows[:, 5] >= 0) == (rows[:, 3] == 2)).all(), (what, "junction words")


# ---- clouds ---------------------------------------------------------------------------------------------------------------------
TWIG_SEED, TWIG_AT_END_SEED = 1, 3  # (checked on the restatement alone: others of 1..5 lose the junction at step 0.02)


def _strip(rng, start, angle_deg, length, count):
    a = np.radians(angle_deg)
    along, across = rng.uniform(0.0, length, count), rng.uniform(-0.002, 0.002, count)
    return np.stack([start[0] + along * np.cos(a) - across * np.sin(a), start[1] + along * np.sin(a) + across * np.cos(a),
                     np.zeros(count)], axis=1)


def twig(seed=TWIG_SEED):
    """a stem of 0.24 m along x, 4 mm across, with a side twig of 0.03 m at mid-length, 2500 samples per metre"""
    rng = np.random.default_rng(seed)
    return np.concatenate([_strip(rng, (0.0, 0.0), 0.0, 0.24, 600), _strip(rng, (0.12, 0.0), 90.0, 0.03, 75)]).astype(np.float32)


def twig_at_end(seed=TWIG_AT_END_SEED):
    """the same stem with the twig at x = 0.225 m, 15 mm before the stem's end: its tip is the longest way from the stem's
    other end (0.255 m against 0.24 m), so the twig holds end b.  The stem's sample nearest to x = 0.24 m comes first: the first
    sweep of CL4 starts there and makes the end at x = 0 end a.  (In a tree end a and end b are the ends of a longest way, so
    the twig's tip can be end b only if what the stem has left past the twig is shorter than the twig: a stub, and a spur.)"""
    rng = np.random.default_rng(seed)
    stem, side = _strip(rng, (0.0, 0.0), 0.0, 0.24, 600), _strip(rng, (0.225, 0.0), 90.0, 0.03, 75)
    last = int(np.argmax(stem[:, 0]))
    stem[[0, last]] = stem[[last, 0]]
    return np.concatenate([stem, side]).astype(np.float32)


def new_cases():
    return {"twig": twig(), "twig_at_end": twig_at_end()}
