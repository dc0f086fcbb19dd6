#!/usr/bin/env python3
"""The coarse registration ("Coarse registration") at scale, on one MI355X.  Run it under one `timeout`.

    python scripts/coarse_register_probe.py [--points N] [--stride 64] [--repeats 2] [--write profiles/coarse_register_probe.md]

The 10 M-point scene as the map against a base of the same size (the scene generated again from the next seed: the room's shell
is the same, its spheres and pillars stand elsewhere; --base-seed-offset 0: the map's own points) under a planted motion of
1.2 rad and 3 m, the map's normals estimated at 0.1 m, the base's estimated by the stage itself.  In one session: the
descriptor stage per side (pcp_coarse_descriptors), the matching (pcp_coarse_match), the scoring of as many frames as the stage
draws hypotheses (pcp_coarse_score), the whole call (pcp_compare_register_coarse) and, as the yardstick, pcp_estimate_normals at
support_radius on the same map: the one existing kernel that walks the same grid at the same radius, for EVERY point where the
descriptor stage has one query per `stride` rows.  Per call the kernels' device time (PCP_K_MISC) and the host's wall clock,
median [min .. max] of --repeats rounds after one warm-up round (the yardstick runs once).  No bar is set.  PCP_HIP_LIBRARY
selects another build of the same ABI.  One JSON line per measurement on stdout; --write also puts the figures into a markdown
file.  Not collected by pytest."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--stride", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--normal-radius", type=float, default=0.1)
    ap.add_argument("--base-seed-offset", type=int, default=1, help="the base is the scene of seed + this (0: the map's own points moved)")
    ap.add_argument("--write", default="")
    args = ap.parse_args()
    import numpy as np

    from pointcloudprocessor_amd import capi, pipeline, synth

    lines = []

    def say(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    say(library=os.environ.get("PCP_HIP_LIBRARY", "default"), points=args.points, stride=args.stride)
    x, y, z, _ = synth.make_cloud(args.points, seed=synth.SEED)
    bx, by, bz, _ = synth.make_cloud(args.points, seed=synth.SEED + args.base_seed_offset)
    # the planted motion takes the base onto the map: 1.2 rad about an oblique axis through the map's centre, then 3 m
    axis = np.array([0.3, -0.5, 0.8]) / math.sqrt(0.98)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(1.2) * K + (1 - math.cos(1.2)) * (K @ K)
    centre = np.array([float(np.mean(x)), float(np.mean(y)), float(np.mean(z))])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = centre - R @ centre + np.array([0.6, 0.64, -0.48]) * 3.0
    inv = np.linalg.inv(T)
    base = (np.stack([bx, by, bz], axis=1).astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    eng = pipeline.HipEngine(0)
    ctx = eng.ctx
    ctx.timing_enable(True)

    def timed(fn):
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return ctx.timing_get(capi.K_MISC)[0], (time.perf_counter() - t0) * 1e3, out

    kw = dict(map_stride=args.stride, base_stride=args.stride, normal_radius=args.normal_radius)
    support = capi.coarse_params(**kw).support_radius
    ctx.upload_cloud(x, y, z)
    ctx.estimate_normals(args.normal_radius)
    ctx.compare_set_base(base)
    names = ("describe_map", "describe_base", "match", "score", "whole")
    rows = {k + s: [] for k in names for s in ("_dev", "_wall")}
    dm = db = whole = None
    for rep in range(1 + args.repeats):
        ctx.compare_set_base_transform(np.eye(4))
        got = [timed(lambda: ctx.coarse_descriptors(capi.CG_MAP, fetch=False, **kw)), timed(lambda: ctx.coarse_descriptors(capi.CG_BASE, fetch=False, **kw))]
        dm, db = got[0][2], got[1][2]
        got.append(timed(lambda: ctx.coarse_match(**kw)))
        pivot = ctx.compare_base_transform()["pivot"]
        frames = np.tile(np.concatenate([np.eye(3).reshape(9), pivot, np.zeros(3)]), (capi.coarse_params(**kw).hypotheses, 1))
        got.append(timed(lambda: ctx.coarse_score(frames, **kw)))
        got.append(timed(lambda: ctx.compare_register_coarse(**kw)))
        whole = got[4][2]
        if rep >= 1:
            for k, g in zip(names, got):
                rows[k + "_dev"].append(g[0])
                rows[k + "_wall"].append(g[1])
    ms = {k: spread(v) for k, v in rows.items()}
    n_dev, n_wall, _ = timed(lambda: ctx.estimate_normals(support))
    piv = np.append(ctx.compare_base_transform()["pivot"], 1.0)
    shift = float(np.linalg.norm((whole["T"] @ piv - T @ piv)[:3]))
    Rr = whole["T"][:3, :3] @ R.T
    angle = math.acos(max(-1.0, min(1.0, (np.trace(Rr) - 1.0) / 2.0)))
    report = {k: whole[k] for k in capi.CG_REPORT}
    say(case="coarse registration", support_radius=support, ms=ms, normals_at_support_ms=dict(device=round(n_dev, 3), wall=round(n_wall, 3)),
        report=report, error_at_pivot_m=shift, error_rad=angle)
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_cg_"], capture_output=True, text=True).stdout.strip()
    say(case="kernel notes", text=notes)
    if args.write:
        def cell(k):
            return "%.3f [%.3f .. %.3f]" % (ms[k]["median"], ms[k]["min"], ms[k]["max"])

        with open(args.write, "w") as fh:
            fh.write("# Coarse registration at scale (`scripts/coarse_register_probe.py`)\n\n"
                     f"One MI355X, {args.points} map points against a base of {len(base)} rows (the scene generated again from seed + {args.base_seed_offset}) under a "
                     f"planted motion of 1.2 rad and 3 m, the map's normals at {args.normal_radius} m, the base's estimated by the stage at the same "
                     f"radius (once: the estimate is kept with the base), stride {args.stride} on both sides, support_radius {support:g}, the other "
                     f"parameters at their defaults.  Milliseconds, median [min .. max] of {args.repeats} rounds after a warm-up; the yardstick ran "
                     "once.  No bar is set.\n\n| call | kernels (PCP_K_MISC) | wall clock |\n|---|---|---|\n"
                     f"| `pcp_coarse_descriptors`, map ({dm['keypoints']} keypoints, {dm['valid']} valid) | {cell('describe_map_dev')} | {cell('describe_map_wall')} |\n"
                     f"| `pcp_coarse_descriptors`, base ({db['keypoints']} keypoints, {db['valid']} valid) | {cell('describe_base_dev')} | {cell('describe_base_wall')} |\n"
                     f"| `pcp_coarse_match` ({report['correspondences']} correspondences) | {cell('match_dev')} | {cell('match_wall')} |\n"
                     f"| `pcp_coarse_score` ({len(frames)} frames) | {cell('score_dev')} | {cell('score_wall')} |\n"
                     f"| `pcp_compare_register_coarse` (the whole call) | {cell('whole_dev')} | {cell('whole_wall')} |\n"
                     f"| `pcp_estimate_normals` at {support:g} m on the same map (every point a query) | {n_dev:.3f} | {n_wall:.3f} |\n\n"
                     f"The report: {json.dumps(report)}.  Against the planted motion the kept frame is {shift:.4f} m off at the base's pivot and "
                     f"{angle:.5f} rad.\n\nKernel notes (`scripts/kernel_notes.py k_cg_`):\n\n```\n" + notes + "\n```\n")


if __name__ == "__main__":
    main()
