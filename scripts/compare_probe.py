#!/usr/bin/env python3
"""The map comparison ("Map comparison") at scale, on one MI355X.  Run it under one `timeout`.

    python scripts/compare_probe.py [--points N] [--repeats 3] [--write profiles/compare_probe.md]

The 10 M-point scene as the map against a base of the same size (the scene generated again from the next seed) at the
default parameters (radius 0.03, half length 0.05, min_points 5), the normals estimated at 0.1 m and turned towards the room's
centre.  In the same session, on the same map: pcp_estimate_normals at radius = the comparison's search radius -- the one
existing kernel that walks the same structure, over one cloud instead of two -- as the yardstick.  Per call the kernels' device
time (PCP_K_MISC) and the host's wall clock, median [min .. max] of --repeats rounds after one warm-up round, and their ratio.
No bar is set.  PCP_HIP_LIBRARY selects another build of the same ABI.  One JSON line per measurement on stdout; --write also
puts the figures into a markdown file.  Not collected by pytest."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--normal-radius", type=float, default=0.1)
    ap.add_argument("--write", default="")
    args = ap.parse_args()
    import numpy as np

    from pointcloudprocessor_amd import capi, pipeline, synth

    lines = []

    def say(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    say(library=os.environ.get("PCP_HIP_LIBRARY", "default"), points=args.points)
    x, y, z, _ = synth.make_cloud(args.points, seed=synth.SEED)
    bx, by, bz, _ = synth.make_cloud(args.points, seed=synth.SEED + 1)
    base = np.stack([bx, by, bz], axis=1)
    radius, half_length = 0.03, 0.05
    f = np.float32
    search = float(np.nextafter(f(math.sqrt(float(f(radius)) ** 2 + float(f(half_length)) ** 2)), f(np.inf)))
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

    ctx.upload_cloud(x, y, z)
    ctx.estimate_normals(args.normal_radius)
    normals = ctx.normals_fetch()["normal"]
    t0 = time.perf_counter()
    ctx.compare_set_base(base)
    say(case="set_base", rows=len(base), wall_ms=round((time.perf_counter() - t0) * 1e3, 3))
    centre = (float(np.mean(x)), float(np.mean(y)), float(np.mean(z)))
    prm = capi.compare_params(radius, half_length, 0.0, 5, 1, centre)
    stats = np.zeros(8, np.int64)

    def compare():
        ctx._check(ctx.lib.pcp_compare(ctx.h, capi.C.byref(prm), capi._ptr(normals), capi._ptr(stats)))
        return stats.copy()

    rows = {k: [] for k in ("compare_dev", "compare_wall", "normals_dev", "normals_wall")}
    for rep in range(1 + args.repeats):
        c_dev, c_wall, st = timed(compare)
        n_dev, n_wall, valid = timed(lambda: ctx.estimate_normals(search))
        if rep >= 1:
            for k, v in zip(rows, (c_dev, c_wall, n_dev, n_wall)):
                rows[k].append(v)
    ms = {k: spread(v) for k, v in rows.items()}
    ratio = round(ms["compare_dev"]["median"] / ms["normals_dev"]["median"], 3) if ms["normals_dev"]["median"] else None
    say(case="compare beside normals", search_radius=search, stats=dict(zip(capi.MC_STATS, (int(v) for v in st))), valid_normals=valid, ms=ms,
        device_ratio=ratio)
    if args.write:
        def cell(k):
            return "%.3f [%.3f .. %.3f]" % (ms[k]["median"], ms[k]["min"], ms[k]["max"])

        with open(args.write, "w") as fh:
            fh.write("# Map comparison at scale (`scripts/compare_probe.py`)\n\n"
                     f"One MI355X, {args.points} map points against a base of {len(base)} rows (the scene generated again from the next seed), radius "
                     f"{radius}, half length {half_length}, min_points 5, normals at {args.normal_radius} m turned towards the room's centre; "
                     f"search radius {search:.7f}.  `pcp_estimate_normals` at that radius on the same map in the same session is the "
                     f"yardstick: the same walk over one cloud.  Milliseconds, median [min .. max] of {args.repeats} rounds after a warm-up.\n\n"
                     "| call | kernels (PCP_K_MISC) | wall clock |\n|---|---|---|\n"
                     f"| `pcp_compare` | {cell('compare_dev')} | {cell('compare_wall')} |\n"
                     f"| `pcp_estimate_normals` at the search radius | {cell('normals_dev')} | {cell('normals_wall')} |\n\n"
                     f"Ratio of the kernels' medians: {ratio}.  Stats: " + ", ".join(f"{k} {int(v)}" for k, v in zip(capi.MC_STATS[:7], st)) + ".\n")


if __name__ == "__main__":
    main()
