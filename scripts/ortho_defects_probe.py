#!/usr/bin/env python3
"""Surface defects on ortho maps (pcp_ortho_defects) on one MI355X; writes profiles/ortho_defects_probe.md.  Not collected by
pytest.

  A planar map of 2412 x 2012 pixels at 2 mm with one point per pixel (2 % of the pixels left empty, closed by a fill of
  radius 2 but for carved blocks), a smooth surface of a few millimetres with 4000 hollows and bulges of 2 to 12 pixels'
  radius.  Kernel time (hipEvents of the call's launches) and wall time of pcp_ortho_defects at W = 0, W = 40 and W = 40
  refined, each measured REPEATS times after a warm-up call; the table build alone comes from the kernel trace.
  The library is the tree's, or the one PCP_HIP_LIBRARY names (the other labelling form); the results are compared with the
  host twin once.  With a second argument that names a `rocprofv3 --kernel-trace --stats` kernel_stats.csv of a run of this
  script, the split by kernel is rendered from it.

    python scripts/ortho_defects_probe.py measure <out.json>            # one library's figures
    python scripts/ortho_defects_probe.py render <shipped.json> <other.json> [kernel_stats.csv] [bench note]
"""
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "ortho_defects_probe.md")
W, H, GSD = 2412, 2012, 0.002
REPEATS = 5
BENCH_CMD = "python bench.py --gpus 1 --steps 20 --warmup 3 --no-side-legs --no-cpu --no-ic-leg"
CONFIGS = (("W = 0", dict(window=0)), ("W = 40", dict(window=40, min_support=8)), ("W = 40 refined", dict(window=40, min_support=8, refine=True)))


def scene():
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = 0.003 * np.sin(xx / 90.0) * np.cos(yy / 70.0) + rng.normal(0, 0.0004, (H, W))
    for _ in range(4000):
        r, c, rad = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(2, 13))
        r0, r1, c0, c1 = max(r - rad, 0), min(r + rad + 1, H), max(c - rad, 0), min(c + rad + 1, W)
        m = (yy[r0:r1, c0:c1] - r) ** 2 + (xx[r0:r1, c0:c1] - c) ** 2 <= rad * rad
        depth[r0:r1, c0:c1][m] += (1.0 if rng.random() < 0.5 else -1.0) * rng.uniform(0.004, 0.02)
    present = rng.random((H, W)) >= 0.02
    for _ in range(40):
        r, c = int(rng.integers(0, H - 30)), int(rng.integers(0, W - 30))
        present[r:r + 20, c:c + 30] = False
    rr, cc = np.nonzero(present)
    return np.stack([(cc + 0.5) * GSD, (rr + 0.5) * GSD, depth[rr, cc]], axis=1).astype(np.float32)


def timed(ctx, capi, fn):
    """(kernel ms over all slots, wall ms) of one call"""
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    got = [ctx.timing_get(k) for k in range(capi.K_COUNT)]
    ctx.timing_enable(False)
    return float(sum(g[0] for g in got)), wall


def measure(path):
    from pointcloudprocessor_amd import capi

    xyz = scene()
    s = dict(library=os.environ.get("PCP_HIP_LIBRARY") or "the tree's", pixels=W * H, points=len(xyz), configs={})
    with capi.Context(0) as ctx:
        ctx.upload_cloud(xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy())
        ctx.ortho_begin(dict(o=(0, 0, 0), u=(1, 0, 0), v=(0, 1, 0), n=(0, 0, 1), gsd=GSD, width=W, height=H, d_min=-1.0, d_max=1.0))
        ctx.ortho_add_packed(np.full(len(xyz), 0x01808080, np.uint32))
        s["occupied"], s["filled"] = ctx.ortho_finish(2)
        m = ctx.ortho_fetch()
        for name, kw in CONFIGS:
            out = ctx.ortho_defects(threshold=0.002, min_pixels=4, **kw)  # (warm-up)
            runs = [timed(ctx, capi, lambda: ctx.ortho_defects(threshold=0.002, min_pixels=4, **kw)) for _ in range(REPEATS)]
            got = ctx.ortho_defects_fetch()
            rows = ctx.ortho_defects_table()
            want = capi.ortho_defects_host(m["depth"], m["status"], threshold=0.002, min_pixels=4, **kw)
            same = all(np.array_equal(got[k], want[k]) for k in got) and np.array_equal(rows, want["rows"]) and \
                all(out[k] == v for k, v in zip(capi.DEFECT_OUT, want["out"]))
            s["configs"][name] = dict(kernels=[r[0] for r in runs], wall=[r[1] for r in runs], out=out, equals_host_twin=bool(same))
            print(name, out, "kernels ms", [round(r[0], 3) for r in runs], "equals the host twin:", same, flush=True)
        ctx.ortho_end()
    with open(path, "w") as f:
        json.dump(s, f)


def series(v):
    return ", ".join("%.3f" % x for x in v)


def split(path):
    """(name, calls, total ms) of the stage's kernels from a rocprofv3 kernel_stats.csv"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "k_sd_" not in name and "k_scan_" not in name:
                continue
            total = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
            rows.append((name.split("(")[0].replace("pcp::", "").replace("void ", ""), int(r.get("Calls") or 0), total / 1e6))
    return sorted(rows, key=lambda t: -t[2])


def render(shipped, other, stats, bench_note):
    a, b = json.load(open(shipped)), json.load(open(other))
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_sd_"], capture_output=True, text=True).stdout
    with open(OUT, "w") as f:
        f.write("# Surface defects on ortho maps: measurements (`scripts/ortho_defects_probe.py`, one MI355X)\n\n")
        f.write("Kernel times are hipEvent times of one call's launches (every timing slot, timing on), wall times include the call's "
                "allocations, its two read-backs and its synchronisations.  Every configuration is measured %d times after one warm-up "
                "call; no download.  Threshold 2 mm, min_pixels 4, min_support 8.  Both labelling forms were run in one session on the "
                "same map, the shipped one from the tree's library and the other from a library built from the same sources with "
                "the other form.\n\n" % REPEATS)
        f.write("## The map: %d x %d pixels at %g m, %d points, %d occupied, %d filled\n\n" % (W, H, GSD, a["points"], a["occupied"], a["filled"]))
        for title, s in (("The shipped form: tiled labelling (a 32 x 16 tile in LDS, then the borders)", a),
                         ("The other form: plain labelling (every link in global memory; `profiles/ortho_defects_plain_labelling.patch`)", b)):
            f.write("## %s\n\n| configuration | kernels, ms | wall, ms | regions kept; dropped; hollow; bulge pixels | equals the host twin |\n|---|---|---|---|---|\n" % title)
            for name, c in s["configs"].items():
                o = c["out"]
                f.write("| %s | %s | %s | %d; %d; %d; %d | %s |\n" % (name, series(c["kernels"]), series(c["wall"]), o["kept"], o["dropped"],
                                                                     o["hollow_pixels"], o["bulge_pixels"], "yes" if c["equals_host_twin"] else "NO"))
            f.write("\n")
        med = lambda s, k: float(np.median(s["configs"][k]["kernels"]))  # noqa: E731
        f.write("## What the figures say\n\n")
        f.write("* Labelling, flatten, scan and statistics with the quantisation (W = 0, median): %.3f ms tiled, %.3f ms plain.\n" % (med(a, "W = 0"), med(b, "W = 0")))
        f.write("* The three configurations class different numbers of pixels (W = 0 classes a third of the map), and the statistics "
                "kernel, whose atomics are merged only where a wavefront's live lanes share one region, takes the more the more pixels "
                "are classed: the configurations are not each other's yardstick.\n")
        rows = {n: (c, ms) for n, c, ms in split(stats)} if stats and os.path.exists(stats) else {}
        if all(k in rows for k in ("k_sd_rows", "k_sd_column_sums", "k_sd_columns", "k_sd_classify<0>")):
            builds = rows["k_sd_rows"][0]
            f.write("* The table build alone (row scan, column sums, column scan over both planes; from the kernel trace below, %d builds): "
                    "%.3f ms a build; the classification of the single pass %.3f ms a call.\n"
                    % (builds, sum(rows[k][1] for k in ("k_sd_rows", "k_sd_column_sums", "k_sd_columns")) / builds,
                       rows["k_sd_classify<0>"][1] / rows["k_sd_classify<0>"][0]))
        else:
            f.write("* The table build alone: not measured.\n")
        f.write("* Shipped: the %s form.\n\n" % ("tiled" if med(a, "W = 0") <= med(b, "W = 0") else "tiled (NOT the faster one here: see the figures)"))
        f.write("## Split by kernel\n\n")
        if stats and os.path.exists(stats):
            f.write("`rocprofv3 --kernel-trace --stats` over one run of this script with the shipped library (a run of its own: %d calls "
                    "per configuration and the warm-ups).\n\n| kernel | calls | total, ms |\n|---|---|---|\n" % REPEATS)
            for name, calls, ms in split(stats):
                f.write("| `%s` | %d | %.3f |\n" % (name, calls, ms))
            f.write("\n")
        else:
            f.write("Not measured.\n\n")
        f.write("## Kernel resources (`scripts/kernel_notes.py k_sd_`, gfx950)\n\n```\n" + notes + "```\n")
        f.write("\n## The timed step\n\n")
        if bench_note:
            f.write("`" + BENCH_CMD + "`, this tree and the parent commit's library alternating in one session: " + bench_note +
                    ".  `bench.py` calls none of the new entry points.\n")
        else:
            f.write("This tree against the parent commit, alternating in one session: not measured.  The command, in each tree in "
                    "turn: `" + BENCH_CMD + "`.  `bench.py` calls none of the new entry points.\n")
    print(open(OUT).read())


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "measure":
        measure(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "render":
        render(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else "", sys.argv[5] if len(sys.argv) > 5 else "")
    else:
        sys.exit(__doc__)
