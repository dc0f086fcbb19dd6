"""Restatement of the fused segmentation label ("Fused segmentation labels") for the tests.

Point i with top list (s_k, f_k), k < M = min(count, 5), and m_k = the mask byte of the pixel keyframe f_k shows it at:
    views = M,  hits = #{k : m_k == 255},  label = floor(sum m_k S_k / sum S_k),  S_k = s_k * 2^26 (an integer)
Two forms: `fuse` with Python ints for one point (checked against fractions.Fraction by the CPU tests) and `fuse_arrays`
with int64 arrays for whole clouds (sums below 2^38: no overflow).  `expected` derives the three arrays from the oracle:
its top lists, its projection for each listed view's pixel, and the uploaded masks."""
from fractions import Fraction

import numpy as np

SCALE_BITS = 26


def score_units(s) -> int:
    """S = s * 2^26 as a Python int; raises if it is not an integer (a score below 2^-3 with low mantissa bits set)."""
    q = Fraction(float(np.float32(s))) * (1 << SCALE_BITS)
    if q.denominator != 1:
        raise ValueError(f"score {s!r} * 2^26 is not an integer")
    return int(q)


def fuse(scores, masks):
    """(label, hits, views) of one point from its listed views' fp32 scores and mask bytes, in exact integers."""
    assert len(scores) == len(masks) <= 5
    if not len(scores):
        return 0, 0, 0
    S = [score_units(s) for s in scores]
    num = sum(int(m) * u for m, u in zip(masks, S))
    return num // sum(S), sum(1 for m in masks if int(m) == 255), len(S)


def fuse_fraction(scores, masks):
    """The definition itself over the rationals: floor of the score-weighted mean of the masks."""
    if not len(scores):
        return 0
    w = [Fraction(float(np.float32(s))) for s in scores]
    mean = sum(Fraction(int(m)) * u for m, u in zip(masks, w)) / sum(w)
    return mean.numerator // mean.denominator


def fuse_arrays(top_score, top_frame, top_mask):
    """(n, 5) lists (entries with frame < 0 are empty) -> label, hits, views uint8[n]."""
    used = top_frame >= 0
    S = np.where(used, top_score.astype(np.float64) * float(1 << SCALE_BITS), 0.0)
    Si = S.astype(np.int64)
    assert np.array_equal(Si.astype(np.float64), S), "a score times 2^26 is not an integer"
    m = np.where(used, top_mask.astype(np.int64), 0)
    num = (m * Si).sum(axis=1)
    den = Si.sum(axis=1)
    views = used.sum(axis=1)
    label = np.where(views > 0, num // np.maximum(den, 1), 0)
    hits = (used & (top_mask == 255)).sum(axis=1)
    return label.astype(np.uint8), hits.astype(np.uint8), views.astype(np.uint8)


def listed_masks(oc, ocam, ocp, x, y, z, poses, masks, top_frame, T_opt=None):
    """m_k of every list entry: the oracle's colour pixel of point i in keyframe f_k, looked up in masks[f_k] (0 for the
    empty entries).  Only the listed (point, keyframe) pairs are projected."""
    n = len(x)
    out = np.zeros((n, 5), np.uint8)
    idx, slot = np.nonzero(top_frame >= 0)
    fr = top_frame[idx, slot]
    order = np.argsort(fr, kind="stable")
    idx, slot, fr = idx[order], slot[order], fr[order]
    bounds = np.searchsorted(fr, np.arange(len(poses) + 1))
    for f in range(len(poses)):
        a, b = bounds[f], bounds[f + 1]
        if a == b:
            continue
        T = None if T_opt is None else (T_opt[f] if np.ndim(T_opt) == 3 else T_opt)
        w2c, _ = oc.pose_to_matrices(poses[f], T)
        i = idx[a:b]
        pix = oc.project_frame(ocam, ocp, w2c, x[i], y[i], z[i])["pixel"]
        assert (pix >= 0).all(), "a listed view has no colour pixel"
        out[i, slot[a:b]] = np.ascontiguousarray(masks[f]).reshape(-1)[pix]
    return out


def expected(oc, ocam, ocp, x, y, z, poses, images, masks, faithful=False, threads=1, T_opt=None):
    """dict(label, hits, views, count, rgb, has) from the oracle (colorize_faithful for PCP_MATCH_RADIUS)."""
    fn = oc.colorize_faithful if faithful else oc.colorize
    ref = fn(ocam, ocp, x, y, z, poses, images, T_opt=T_opt, threads=threads)
    tm = listed_masks(oc, ocam, ocp, x, y, z, poses, masks, ref["top_frame"], T_opt=T_opt)
    label, hits, views = fuse_arrays(ref["top_score"], ref["top_frame"], tm)
    assert np.array_equal(views, np.minimum(ref["count"], 5))
    return dict(label=label, hits=hits, views=views, count=ref["count"], rgb=ref["rgb"], has=ref["has"], top_mask=tm,
                top_score=ref["top_score"], top_frame=ref["top_frame"])
