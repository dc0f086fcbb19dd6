#!/usr/bin/env python3
"""Crack directions on the map (pcp_crack_directions) on one MI355X; writes profiles/crack_direction_probe.md.  Not collected by
pytest.

  The scene of scripts/crack_fuse_probe.py: a noisy tilted wall of POINTS map points (default 2 M) seen at 1920 x 1080,
  thin-crack masks, ADDED keyframes (default 16) added; min_views 1, radius 0.02.
  Wall time and kernel time of pcp_crack_components (the yardstick: it walks the same links) and of pcp_crack_directions on the
  same state in the same session; pcp_crack_directions runs the component stage first, so the difference is the stage's own
  kernel (k_cd_directions).  Registers, LDS and scratch from scripts/kernel_notes.py.  With a fourth argument the measurements are
  saved there as JSON, or, if that file exists, the file is rendered from it without touching a GPU.

    python scripts/crack_direction_probe.py [points] [added] [the bench figures to quote, or ""] [measurements json]
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

POINTS = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
ADDED = int(sys.argv[2]) if len(sys.argv) > 2 else 16
BENCH_NOTE = sys.argv[3] if len(sys.argv) > 3 else ""
KEEP = sys.argv[4] if len(sys.argv) > 4 else ""
OUT = os.path.join(ROOT, "profiles", "crack_direction_probe.md")
W, H = 1920, 1080
REPEATS = 5
BENCH_CMD = "python bench.py --gpus 1 --steps 20 --warmup 3 --no-side-legs --no-cpu --no-ic-leg"


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


def measure():
    import _crack_width_ref as ref
    import _mask_edt_ref as edt_ref
    from pointcloudprocessor_amd import capi

    rng = np.random.default_rng(1)
    C = capi.C
    with capi.Context(0) as ctx:
        shape = (H, W)
        ctx.set_camera(capi.camera_from_dict(ref.camera(shape)), capi.default_cull_params())
        _, c2w = capi.pose_to_matrices(ref.IDENTITY_POSE)
        cloud = ref.wall_cloud(shape, seed=1, density=POINTS / (H * W), c2w=c2w)
        ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
        poses = np.tile(ref.IDENTITY_POSE, (ADDED, 1))
        poses[:, :3] = rng.uniform(-0.05, 0.05, (ADDED, 3))
        ctx.set_frames(poses)
        for f in range(ADDED):
            ctx.upload_mask(f, edt_ref.crack_mask(shape, seed=100 + f, cracks=8))
        ctx.crack_fuse_begin()
        for f in range(ADDED):
            ctx.crack_fuse_add(f)
        prm = capi.CrackLinkParams(1, 0.02)

        def components():
            ctx._check(ctx.lib.pcp_crack_components(ctx.h, C.byref(prm), None, None, None))

        def directions():
            ctx._check(ctx.lib.pcp_crack_directions(ctx.h, C.byref(prm), None, None, None, None, None, None))

        components()  # (warm-up: it allocates the grid)
        directions()
        comp = [timed(ctx, capi, components) for _ in range(REPEATS)]
        dirs = [timed(ctx, capi, directions) for _ in range(REPEATS)]
        t0 = time.perf_counter()
        out = ctx.crack_directions(1, 0.02)  # (once more, with the per-point arrays and the fetch)
        wall_all = (time.perf_counter() - t0) * 1e3
        ctx.crack_fuse_end()
    valid = out["tangent"].any(axis=1)
    return dict(points=len(cloud), added=ADDED, crack_points=int(out["crack_points"]), cracks=int(out["cracks"]), radius=0.02,
                kernels_c=[c[0] for c in comp], wall_c=[c[1] for c in comp], kernels_d=[d[0] for d in dirs], wall_d=[d[1] for d in dirs],
                wall_with_fetches=wall_all, tangents=int(valid.sum()), most_links=int(out["links"].max(initial=0)),
                mean_links=float(out["links"][out["links"] > 0].mean()) if (out["links"] > 0).any() else 0.0,
                ordered_links=float(out["link_count"].sum()), axes=int(out["axis"].any(axis=1).sum()),
                median_anisotropy=float(np.median(out["anisotropy"][valid])) if valid.any() else 0.0)


def series(v):
    return ", ".join("%.3f" % x for x in v)


def main():
    if KEEP and os.path.exists(KEEP):
        with open(KEEP) as f:
            s = json.load(f)
    else:
        s = measure()
        if KEEP:
            with open(KEEP, "w") as f:
                json.dump(s, f)
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_cd_", "k_cc_union", "k_cc_stats"],
                           capture_output=True, text=True).stdout
    kc, kd = float(np.median(s["kernels_c"])), float(np.median(s["kernels_d"]))
    with open(OUT, "w") as f:
        f.write("# Crack directions on the map: measurements (`scripts/crack_direction_probe.py`, one MI355X)\n\n")
        f.write("Kernel times are hipEvent times of one call's launches (every timing slot, timing on), wall times include the call's "
                "synchronisations.  Every call is measured %d times after one warm-up call of each; no download.  `pcp_crack_directions` runs "
                "the component stage first, so its own kernel is the difference to `pcp_crack_components`, the yardstick: both walk the same "
                "links.  The 10 M-point scene was not run: not measured.\n\n" % REPEATS)
        f.write("## The wall (the scene of `crack_fuse_probe.py`, %d x %d, thin-crack masks)\n\n" % (W, H))
        f.write("| what | figure |\n|---|---|\n")
        f.write("| map points; keyframes added; crack points; cracks | %d; %d; %d; %d |\n" % (s["points"], s["added"], s["crack_points"], s["cracks"]))
        f.write("| links per crack point: mean; most; ordered links in all | %.1f; %d; %.0f |\n" % (s["mean_links"], s["most_links"], s["ordered_links"]))
        f.write("| `pcp_crack_components` (min_views 1, radius %g): kernels, ms | %s |\n" % (s["radius"], series(s["kernels_c"])))
        f.write("| ... wall, ms | %s |\n" % series(s["wall_c"]))
        f.write("| `pcp_crack_directions` on the same state: kernels, ms | %s |\n" % series(s["kernels_d"]))
        f.write("| ... wall, ms | %s |\n" % series(s["wall_d"]))
        f.write("| the stage's own kernel (the difference of the medians) | %.3f ms |\n" % (kd - kc))
        f.write("| ... over the yardstick's kernels (median) | %.2f |\n" % ((kd - kc) / kc if kc > 0 else float("nan")))
        f.write("| the call with the three per-point arrays, the fetch and the axes: wall | %.3f ms |\n" % s["wall_with_fetches"])
        f.write("| points with a tangent; their median anisotropy; cracks with an axis | %d; %.3f; %d |\n" % (s["tangents"], s["median_anisotropy"], s["axes"]))
        f.write("\n## Kernel resources (`scripts/kernel_notes.py k_cd_ k_cc_union k_cc_stats`, gfx950)\n\n```\n" + notes + "```\n")
        f.write("\n## The timed step\n\n")
        if BENCH_NOTE:
            f.write("`" + BENCH_CMD + "`, this tree and the parent commit's library alternating in one session: " + BENCH_NOTE +
                    ".  `bench.py` calls none of the new entry points.\n")
        else:
            f.write("This tree against the parent commit, alternating in one session: not measured.  The command, in each tree in "
                    "turn: `" + BENCH_CMD + "`.  `bench.py` calls none of the new entry points.\n")
    print(open(OUT).read())


if __name__ == "__main__":
    main()
