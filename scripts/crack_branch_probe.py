#!/usr/bin/env python3
"""Crack branches on the map (pcp_crack_branches) on one MI355X; writes profiles/crack_branch_probe.md.  Not collected by pytest.

  wall   the 2 M-point wall scene of scripts/crack_direction_probe.py (1920 x 1080, thin-crack masks, ADDED keyframes added;
         min_views 1, radius 0.02, step 0.04, prune 0.08): region-like cracks
  lines  the LINES straight bands (default 50; 0: the scene is left out and the file says so) of scripts/crack_skeleton_probe.py
         seen through the 64 x 64 scene harness of the GPU tests (radius 0.005, step 0.01, prune 0.02): line-like cracks
  Per scene, in one session, REPEATS calls each after a warm-up, kernel time by hipEvent (every timing slot) and wall time:
  pcp_crack_skeleton; pcp_crack_branches, which runs that stage first, so its own share is the difference of the two; and, as the
  yardstick, pcp_crack_directions' own kernel (its difference to pcp_crack_components): k_cb_branches is that walk with one more
  compare.  The host share of the stage (the graph part, its download and its upload) is the difference of the wall times minus
  the difference of the kernel times.  Registers, LDS and scratch from scripts/kernel_notes.py.  With a fifth argument the
  measurements are saved there as JSON, or, if that file exists, the file is rendered from it without touching a GPU.

    python scripts/crack_branch_probe.py [points] [added] [lines] [the bench figures to quote, or ""] [measurements json]
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
LINES = int(sys.argv[3]) if len(sys.argv) > 3 else 50
BENCH_NOTE = sys.argv[4] if len(sys.argv) > 4 else ""
KEEP = sys.argv[5] if len(sys.argv) > 5 else ""
OUT = os.path.join(ROOT, "profiles", "crack_branch_probe.md")
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


def stage(ctx, capi, radius, step, prune):
    C = capi.C
    prm = capi.CrackLinkParams(1, radius)
    calls = dict(
        components=lambda: ctx._check(ctx.lib.pcp_crack_components(ctx.h, C.byref(prm), None, None, None)),
        directions=lambda: ctx._check(ctx.lib.pcp_crack_directions(ctx.h, C.byref(prm), None, None, None, None, None, None)),
        skeleton=lambda: ctx._check(ctx.lib.pcp_crack_skeleton(ctx.h, C.byref(prm), C.c_float(step), None, None, None)),
        branches=lambda: ctx._check(ctx.lib.pcp_crack_branches(ctx.h, C.byref(prm), C.c_float(step), C.c_float(prune), None, None, None)))
    out = dict(radius=radius, step=step, prune=prune)
    for name, fn in calls.items():
        fn()  # (warm-up: the first call allocates)
        runs = [timed(ctx, capi, fn) for _ in range(REPEATS)]
        out["kernels_" + name], out["wall_" + name] = [r[0] for r in runs], [r[1] for r in runs]
    res = ctx.crack_branches(1, radius, step, prune)  # (once more, with the per-point array and the fetches: for the counts)
    cracks = res["cracks"]
    out.update(crack_points=int((res["branch"] != -1).sum()), cracks=len(cracks), branches=len(res["ids"]), bridges=int(cracks[:, 1].sum()),
               junctions_kept=int(cracks[:, 2].sum()), pruned_branches=int(cracks[:, 4].sum()), pruned_nodes=int(cracks[:, 5].sum()),
               pruned_points=int(cracks[:, 6].sum()), edges=len(res["edge_branch"]), kept_length_m=float(res["kept_length_m"].sum()))
    return out


def measure():
    import _crack_width_ref as ref
    import _mask_edt_ref as edt_ref
    from pointcloudprocessor_amd import capi
    from test_crack_fuse_gpu import CASE_SHAPE, _case_scene

    m = {}
    rng = np.random.default_rng(1)
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
        m["wall"] = dict(points=len(cloud), added=ADDED, **stage(ctx, capi, 0.02, 0.04, 0.08))
        ctx.crack_fuse_end()
    if LINES == 0:
        return m
    with capi.Context(0) as ctx:
        bands = []
        for k in range(LINES):
            r = np.random.default_rng(1000 + k)
            bands.append(np.stack([r.uniform(0.0, 2.0, 4000), 0.05 * k + r.uniform(-0.002, 0.002, 4000), np.zeros(4000)], axis=1))
        cloud, poses, masks = _case_scene(np.concatenate(bands).astype(np.float32))
        cam = ref.camera(CASE_SHAPE)
        cam.update(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
        cull = capi.default_cull_params()
        cull.enable_depth_buffer_culling = 0
        ctx.set_camera(capi.camera_from_dict(cam), cull)
        ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
        ctx.set_frames(np.asarray(poses, np.float64))
        for f, mask in enumerate(masks):
            ctx.upload_mask(f, mask)
        ctx.crack_fuse_begin()
        for f in range(len(masks)):
            ctx.crack_fuse_add(f, 0, 150)
        m["lines"] = dict(points=len(cloud), added=len(masks), lines=LINES, **stage(ctx, capi, 0.005, 0.01, 0.02))
        ctx.crack_fuse_end()
    return m


def series(v):
    return ", ".join("%.3f" % x for x in v)


def table(f, s):
    med = lambda key: float(np.median(s[key]))  # noqa: E731
    own_k = med("kernels_branches") - med("kernels_skeleton")
    own_wall = med("wall_branches") - med("wall_skeleton")
    yard = med("kernels_directions") - med("kernels_components")
    f.write("| what | figure |\n|---|---|\n")
    f.write("| map points; keyframes added; crack points; cracks | %d; %d; %d; %d |\n" % (s["points"], s["added"], s["crack_points"], s["cracks"]))
    f.write("| radius; step; prune | %g; %g; %g |\n" % (s["radius"], s["step"], s["prune"]))
    for name in ("skeleton", "branches", "components", "directions"):
        f.write("| `pcp_crack_%s`: kernels, ms | %s |\n| ... wall, ms | %s |\n" % (name, series(s["kernels_" + name]), series(s["wall_" + name])))
    f.write("| the stage's own kernels (branches - skeleton, medians) | %.3f ms |\n" % own_k)
    f.write("| the yardstick, `k_cd_directions` (directions - components, medians) | %.3f ms |\n" % yard)
    f.write("| ... the stage's kernels over the yardstick | %.2f |\n" % (own_k / yard if yard > 0 else float("nan")))
    f.write("| the stage's host share (graph part, download, upload: wall difference - kernel difference) | %.3f ms |\n" % (own_wall - own_k))
    f.write("| edges; branches; bridges; kept junctions | %d; %d; %d; %d |\n" % (s["edges"], s["branches"], s["bridges"], s["junctions_kept"]))
    f.write("| pruned branches; nodes; points | %d; %d; %d |\n" % (s["pruned_branches"], s["pruned_nodes"], s["pruned_points"]))
    f.write("| kept length, all cracks | %.3f m |\n" % s["kept_length_m"])


def main():
    if KEEP and os.path.exists(KEEP):
        with open(KEEP) as f:
            m = json.load(f)
    else:
        m = measure()
        if KEEP:
            with open(KEEP, "w") as f:
                json.dump(m, f)
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_cb_", "k_cd_"], capture_output=True, text=True).stdout
    with open(OUT, "w") as f:
        f.write("# Crack branches on the map: measurements (`scripts/crack_branch_probe.py`, one MI355X)\n\n")
        f.write("Kernel times are hipEvent times of one call's launches (every timing slot, timing on), wall times include the call's "
                "synchronisations.  Every call is measured %d times after one warm-up call of each; no download.  `pcp_crack_branches` runs "
                "the skeleton stage first, so its own share is the difference to `pcp_crack_skeleton`; the yardstick is `pcp_crack_directions`' "
                "own kernel, its difference to `pcp_crack_components`.\n\n" % REPEATS)
        f.write("## The wall (the scene of `crack_direction_probe.py`, %d x %d, thin-crack masks)\n\n" % (W, H))
        table(f, m["wall"])
        if "lines" in m:
            f.write("\n## %d straight bands of 2 m x 4 mm, 4 000 points each (the 64 x 64 scene harness of the GPU tests)\n\n" % m["lines"]["lines"])
            table(f, m["lines"])
        else:
            f.write("\n## Straight bands of 2 m x 4 mm (the line-like scene of `crack_skeleton_probe.py`)\n\nNot measured: the scene was left out of "
                    "this run (`lines` 0).  The command: `python scripts/crack_branch_probe.py 2000000 16 50`.\n")
        f.write("\n## Kernel resources (`scripts/kernel_notes.py k_cb_ k_cd_`, gfx950)\n\n```\n" + notes + "```\n")
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
