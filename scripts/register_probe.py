#!/usr/bin/env python3
"""The map registration ("Map registration") at scale, on one MI355X.  Run it under one `timeout`.

    python scripts/register_probe.py [--points N] [--repeats 3] [--write profiles/register_probe.md]

The 10 M-point scene as the map against a base of the same size (the scene generated again from the next seed), the scene of
compare_probe.py, the normals estimated at 0.1 m.  In the same session, on the same map and base: one evaluation of the
registration's sums (pcp_compare_register_sums: the grid over both clouds, the search kernel, the fold) at match_radius = the
comparison's search radius, beside pcp_compare at the default parameters -- the one existing kernel that walks the same grid of
the same two clouds -- as the yardstick.  Then the whole loop (pcp_compare_register) from the identity with its iteration count.
Per call the kernels' device time (PCP_K_MISC) and the host's wall clock, median [min .. max] of --repeats rounds after one
warm-up round, and their ratio.  No bar is set.  PCP_HIP_LIBRARY selects another build of the same ABI.  One JSON line per
measurement on stdout; --write also puts the figures into a markdown file.  Not collected by pytest."""
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
    ctx.compare_set_base(base)
    centre = (float(np.mean(x)), float(np.mean(y)), float(np.mean(z)))
    reg = dict(match_radius=search, max_plane_distance=0.02)
    prm = capi.compare_params(radius, half_length, 0.0, 5, 1, centre)
    stats = np.zeros(8, np.int64)

    def compare():  # (without the fetch: the kernels and their launch alone)
        ctx._check(ctx.lib.pcp_compare(ctx.h, capi.C.byref(prm), None, capi._ptr(stats)))

    rows = {k: [] for k in ("sums_dev", "sums_wall", "compare_dev", "compare_wall", "loop_dev", "loop_wall")}
    sums = loop = None
    for rep in range(1 + args.repeats):
        ctx.compare_set_base_transform(np.eye(4))
        s_dev, s_wall, sums = timed(lambda: ctx.compare_register_sums(**reg))
        c_dev, c_wall, _ = timed(compare)
        l_dev, l_wall, loop = timed(lambda: ctx.compare_register(**reg))
        if rep >= 1:
            for k, v in zip(rows, (s_dev, s_wall, c_dev, c_wall, l_dev, l_wall)):
                rows[k].append(v)
    ms = {k: spread(v) for k, v in rows.items()}
    ratio = round(ms["sums_dev"]["median"] / ms["compare_dev"]["median"], 3) if ms["compare_dev"]["median"] else None
    shift = float(np.linalg.norm(loop["T"][:3, 3] + loop["T"][:3, :3] @ np.array(centre) - np.array(centre)))
    say(case="register beside compare", match_radius=search, pairs=int(sums[58]), ms=ms, device_ratio=ratio, iterations=loop["iterations"],
        status=loop["status"], dof=loop["dof"], rms=loop["rms"], shift_at_centre=shift, log=loop["log"].tolist())
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_rg"], capture_output=True, text=True).stdout.strip()
    say(case="kernel notes", text=notes)
    if args.write:
        def cell(k):
            return "%.3f [%.3f .. %.3f]" % (ms[k]["median"], ms[k]["min"], ms[k]["max"])

        per = ms["loop_dev"]["median"] / max(1, loop["iterations"])
        with open(args.write, "w") as fh:
            fh.write("# Map registration at scale (`scripts/register_probe.py`)\n\n"
                     f"One MI355X, {args.points} map points against a base of {len(base)} rows (the scene generated again from the next seed), "
                     f"normals at {args.normal_radius} m, match_radius {search:.7f} (the comparison's search radius at its defaults), "
                     f"max_plane_distance 0.02, sample_stride 1.  `pcp_compare` at radius {radius}, half length {half_length} on the same map and "
                     f"base in the same session is the yardstick: the same grid over the same two clouds.  Milliseconds, median [min .. max] of "
                     f"{args.repeats} rounds after a warm-up.\n\n"
                     "| call | kernels (PCP_K_MISC) | wall clock |\n|---|---|---|\n"
                     f"| `pcp_compare_register_sums` (one evaluation) | {cell('sums_dev')} | {cell('sums_wall')} |\n"
                     f"| `pcp_compare` | {cell('compare_dev')} | {cell('compare_wall')} |\n"
                     f"| `pcp_compare_register` (the loop, {loop['iterations']} iterations) | {cell('loop_dev')} | {cell('loop_wall')} |\n\n"
                     f"Ratio of the kernels' medians, one evaluation over `pcp_compare`: {ratio}.  The loop: {per:.3f} ms of kernels per "
                     f"iteration (the transform kernel included), status {loop['status']}, dof {loop['dof']}, {int(sums[58])} pairs at the "
                     f"identity, rms {loop['rms']:.6f} m, the room's centre moved by {shift:.6f} m.\n\n"
                     "Kernel notes (`scripts/kernel_notes.py k_rg`):\n\n```\n" + notes + "\n```\n")


if __name__ == "__main__":
    main()
