"""Restatement of smoothColorsWithLocalRegion (PointCloudProcessor.cpp:634-703) as DESIGN.md LS1-LS7 pin it.

numpy + scipy.spatial.cKDTree: the candidates of a query come from query_ball_point(r * 1.001) (a superset), the
neighbour rule LS2 is then applied exactly as written -- fp32 differences, squares and sums, compared in fp64 with
(double)r * (double)r --, w = np.float32(1) / np.float32(1 + d2) (LS3), m = w * 2^24 as int64 and exact integer floors
(LS4).  Words are r | g<<8 | b<<16 | has<<24; the has bit of the input is not read.
"""
from __future__ import annotations

import numpy as np


def split(words):
    w = np.asarray(words, np.uint32)
    return (w & 0xFF).astype(np.int64), ((w >> 8) & 0xFF).astype(np.int64), ((w >> 16) & 0xFF).astype(np.int64)


def pack(r, g, b):
    r, g, b = (np.asarray(v, np.uint32) for v in (r, g, b))
    has = ((r | g | b) != 0).astype(np.uint32)
    return r | (g << 8) | (b << 16) | (has << 24)


def neighbour_weights(x, y, z, i, cand, radius):
    """LS2 + LS3 for query i against candidate indices `cand`: (mask, m) with m = w * 2^24 (int64)."""
    f = np.float32
    dx = (x[cand] - x[i]).astype(f)
    dy = (y[cand] - y[i]).astype(f)
    dz = (z[cand] - z[i]).astype(f)
    d2 = ((dx * dx).astype(f) + (dy * dy).astype(f)).astype(f)
    d2 = (d2 + (dz * dz).astype(f)).astype(f)
    inside = d2.astype(np.float64) <= np.float64(np.float32(radius)) * np.float64(np.float32(radius))
    w = (f(1.0) / (f(1.0) + d2).astype(f)).astype(f)
    m = (w.astype(np.float64) * 16777216.0).astype(np.int64)
    return inside, m


def smooth_local(x, y, z, words, radius, queries=None):
    """Smoothed words of the points `queries` (default: all, then the whole output array is returned with the
    non-finite points keeping their word); with `queries` given, only those outputs, in that order."""
    from scipy.spatial import cKDTree

    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    z = np.asarray(z, np.float32)
    words = np.asarray(words, np.uint32)
    r = float(np.float32(radius))
    if not (np.isfinite(r) and 0.0 < r <= 1.0):
        raise ValueError("radius must be finite with 0 < radius <= 1 (LS7)")
    n = len(x)
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    fidx = np.nonzero(finite)[0]
    cr, cg, cb = split(words)
    all_out = queries is None
    q = np.arange(n) if all_out else np.asarray(queries, np.int64)
    out = words.copy() if all_out else words[q].copy()
    if len(fidx) == 0:
        return out
    pts = np.stack([x[fidx], y[fidx], z[fidx]], axis=1).astype(np.float64)
    tree = cKDTree(pts)
    qf = [(k, i) for k, i in enumerate(q) if finite[i]]
    if not qf:
        return out
    balls = tree.query_ball_point(pts[np.searchsorted(fidx, [i for _, i in qf])], r * 1.001)
    for (k, i), ball in zip(qf, balls):
        cand = fidx[np.asarray(ball, np.int64)]
        inside, m = neighbour_weights(x, y, z, i, cand, r)
        c = cand[inside]
        m = m[inside]
        sm = int(m.sum())
        vals = [int((m * ch[c]).sum()) // sm for ch in (cr, cg, cb)]
        out[k] = pack(*vals)
    return out


def brute_force_fraction(x, y, z, words, radius):
    """LS1-LS7 with exact rational arithmetic (fractions.Fraction) over every pair: the restatement's own check."""
    from fractions import Fraction

    f = np.float32
    n = len(x)
    out = np.asarray(words, np.uint32).copy()
    cr, cg, cb = split(words)
    r2 = Fraction(float(np.float32(radius))) ** 2
    fin = [bool(np.isfinite(x[i]) and np.isfinite(y[i]) and np.isfinite(z[i])) for i in range(n)]
    for i in range(n):
        if not fin[i]:
            continue
        sw = Fraction(0)
        s = [Fraction(0)] * 3
        for j in range(n):
            if not fin[j]:
                continue
            dx, dy, dz = f(x[j] - x[i]), f(y[j] - y[i]), f(z[j] - z[i])
            d2 = f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
            if Fraction(float(d2)) <= r2:
                w = Fraction(float(f(f(1.0) / f(f(1.0) + d2))))
                sw += w
                s = [s[0] + w * int(cr[j]), s[1] + w * int(cg[j]), s[2] + w * int(cb[j])]
        vals = [int(v / sw) for v in s]  # floor: both non-negative
        out[i] = pack(*vals)
    return out
