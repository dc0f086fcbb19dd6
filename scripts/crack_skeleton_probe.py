#!/usr/bin/env python3
"""Crack skeletons on the map (pcp_crack_skeleton) on one MI355X; writes profiles/crack_skeleton_probe.md.  Not collected by pytest.

  Two scenes:
    wall   the scene of scripts/crack_length_probe.py: a noisy tilted wall of POINTS map points (default 2 M) seen at
           1920 x 1080, thin-crack masks, ADDED keyframes (default 16) added; min_views 1, radius 0.02, step 0.04.  Its cracks
           are regions, many points wide;
    lines  LINES straight bands (default 50) of 2 m x 4 mm with 4 000 points each, 5 cm apart, seen through the 64 x 64 scene
           harness of the GPU tests; min_views 1, radius 0.005, step 0.01.  Its cracks are line-like.
  Per scene: wall time and kernel time of pcp_crack_components (the yardstick: each of the stage's two walks over the links has
  that stage's shape), of pcp_crack_lengths and of pcp_crack_skeleton, which runs both first: the difference to
  pcp_crack_lengths is the stage's own; the node, edge and crack counts; the doublings of the edge set (0 unless the set was
  too small: the call's timed launches minus those of pcp_crack_lengths and the stage's 8 brackets, over 2).
  The split of the stage's kernel time by kernel needs the kernels' names: pass the .csv of
  `rocprofv3 --kernel-trace --stats -- python scripts/crack_skeleton_probe.py ...` as the fifth argument, or leave it out (the
  file then says so).  With a sixth argument the measurements are saved there as JSON, or, if that file exists, the file is
  rendered from it without touching a GPU.

    python scripts/crack_skeleton_probe.py [points] [added] [lines] [the bench figures to quote, or ""] [kernel stats csv] [measurements json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

POINTS = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
ADDED = int(sys.argv[2]) if len(sys.argv) > 2 else 16
LINES = int(sys.argv[3]) if len(sys.argv) > 3 else 50
BENCH_NOTE = sys.argv[4] if len(sys.argv) > 4 else ""
STATS = sys.argv[5] if len(sys.argv) > 5 else ""
KEEP = sys.argv[6] if len(sys.argv) > 6 else ""
OUT = os.path.join(ROOT, "profiles", "crack_skeleton_probe.md")
W, H = 1920, 1080
OWN_BRACKETS = 8  # band; union; flatten and scan; ids; nodes; clear; edges; compact, degree, summary and loops
BENCH_CMD = "python bench.py --gpus 1 --steps 20 --warmup 3 --no-side-legs --no-cpu --no-ic-leg"


def timed(ctx, capi, fn):
    """(kernel ms over all slots, timed launches, wall ms, result) of one call"""
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    got = [ctx.timing_get(k) for k in range(capi.K_COUNT)]
    ctx.timing_enable(False)
    return float(sum(g[0] for g in got)), int(sum(g[1] for g in got)), wall, out


def kernel_split(path):
    """name -> (calls, total ms, shortest ms, longest ms) of the k_cs_, k_cc_ and k_cl_ kernels in a rocprofv3 kernel stats csv"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if any(p in name for p in ("k_cs_", "k_cc_", "k_cl_")):
                out[name.split("(")[0].replace("void ", "")] = (int(row["Calls"]), float(row["TotalDurationNs"]) / 1e6, float(row["MinNs"]) / 1e6,
                                                                      float(row["MaxNs"]) / 1e6)
    return out


def stage(ctx, capi, radius, step):
    """the three calls on the live accumulation, each timed once after a warm-up of the component stage (it allocates the grid)"""
    ctx.crack_components(1, radius)
    ms_c, _, wall_c, comp = timed(ctx, capi, lambda: ctx.crack_components(1, radius))
    prm = capi.CrackLinkParams(1, radius)
    C = capi.C

    def lengths():
        ctx._check(ctx.lib.pcp_crack_lengths(ctx.h, C.byref(prm), None, None, None))

    kn, ke = C.c_int64(), C.c_int64()

    def skeleton():
        ctx._check(ctx.lib.pcp_crack_skeleton(ctx.h, C.byref(prm), C.c_float(step), None, C.byref(kn), C.byref(ke)))

    ms_l, n_l, wall_l, _ = timed(ctx, capi, lengths)
    ms_s, n_s, wall_s, _ = timed(ctx, capi, skeleton)
    t0 = time.perf_counter()
    out = ctx.crack_skeleton(1, radius, step)  # (once more, with the node array and the fetches: for the counts)
    wall_all = (time.perf_counter() - t0) * 1e3
    cracks = out["cracks"]
    return dict(radius=radius, step=step, crack_points=int(comp["crack_points"]), cracks=int(comp["components"]), wall_c=wall_c, kernels_c=ms_c,
                wall_l=wall_l, kernels_l=ms_l, wall_s=wall_s, kernels_s=ms_s, doublings=(n_s - n_l - OWN_BRACKETS) // 2, nodes=int(kn.value),
                edges=int(ke.value), wall_with_fetches=wall_all, ends=int(cracks[:, 2].sum()), junctions=int(cracks[:, 3].sum()),
                loops=int(cracks[:, 4].sum()), most_nodes=int(cracks[:, 0].max()) if len(cracks) else 0,
                length_m=float(out["skeleton_length_m"].sum()))


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
        m["wall"] = dict(points=len(cloud), added=ADDED, **stage(ctx, capi, 0.02, 0.04))
        ctx.crack_fuse_end()
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
        m["lines"] = dict(points=len(cloud), added=len(masks), lines=LINES, **stage(ctx, capi, 0.005, 0.01))
        ctx.crack_fuse_end()
    return m


def table(f, s):
    own_wall, own_k = s["wall_s"] - s["wall_l"], s["kernels_s"] - s["kernels_l"]
    f.write("| what | figure |\n|---|---|\n")
    f.write("| map points; keyframes added; crack points; cracks | %d; %d; %d; %d |\n" % (s["points"], s["added"], s["crack_points"], s["cracks"]))
    f.write("| `pcp_crack_components` (min_views 1, radius %g), the yardstick: wall; kernels | %.3f ms; %.3f ms |\n" % (s["radius"], s["wall_c"], s["kernels_c"]))
    f.write("| `pcp_crack_lengths` on the same state, no download (it runs the component stage first): wall; kernels | %.3f ms; %.3f ms |\n"
            % (s["wall_l"], s["kernels_l"]))
    f.write("| `pcp_crack_skeleton` (step %g), no download (it runs both first): wall; kernels | %.3f ms; %.3f ms |\n" % (s["step"], s["wall_s"], s["kernels_s"]))
    f.write("| the stage's own share (the difference to `pcp_crack_lengths`): wall; kernels | %.3f ms; %.3f ms |\n" % (own_wall, own_k))
    f.write("| ... over the yardstick's kernels | %.2f |\n" % (own_k / s["kernels_c"] if s["kernels_c"] > 0 else float("nan")))
    f.write("| the call with the node array and the three fetches: wall | %.3f ms |\n" % s["wall_with_fetches"])
    f.write("| nodes; unique edges; the most nodes in one crack | %d; %d; %d |\n" % (s["nodes"], s["edges"], s["most_nodes"]))
    f.write("| ends; junctions; loops; skeleton length over all cracks | %d; %d; %d; %.3f m |\n" % (s["ends"], s["junctions"], s["loops"], s["length_m"]))
    f.write("| doublings of the edge set (it starts at four slots per node) | %d |\n" % s["doublings"])


def main():
    if KEEP and os.path.exists(KEEP):
        with open(KEEP) as f:
            m = json.load(f)
    else:
        m = measure()
        if KEEP:
            with open(KEEP, "w") as f:
                json.dump(m, f)
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_cs_"], capture_output=True, text=True).stdout
    with open(OUT, "w") as f:
        f.write("# Crack skeletons on the map: measurements (`scripts/crack_skeleton_probe.py`, one MI355X)\n\n")
        f.write("Kernel times are hipEvent times of one call's launches (every timing slot, timing on), wall times include the call's "
                "synchronisations.  Every call is measured once, after one warm-up call of the component stage.  `pcp_crack_skeleton` runs "
                "the length stage first and inherits its cost: on region-like cracks that is nearly all of the call (the plain round "
                "schedule of `k_cl_relax`; DESIGN.md, \"Crack lengths on the map\").  The 10 M-point scene was not run: not measured.\n\n")
        f.write("## The wall: region-like cracks (the scene of `crack_length_probe.py`, %d x %d, thin-crack masks)\n\n" % (W, H))
        table(f, m["wall"])
        f.write("\n## %d straight bands of 2 m x 4 mm, 4 000 points each: line-like cracks (the 64 x 64 scene harness of the GPU tests)\n\n" % m["lines"]["lines"])
        table(f, m["lines"])
        if STATS:
            split = kernel_split(STATS)
            f.write("\n## The kernels by name (`rocprofv3 --kernel-trace --stats` over the run of this script that made the figures above: both "
                    "scenes, every call of it)\n\n")
            f.write("| kernel | calls | total ms | shortest ms | longest ms |\n|---|---|---|---|---|\n")
            for name, (calls, ms, lo, hi) in sorted(split.items(), key=lambda kv: -kv[1][1]):
                f.write("| `%s` | %d | %.3f | %.3f | %.3f |\n" % (name, calls, ms, lo, hi))
        else:
            f.write("\nThe stage's kernel time split by kernel: not measured (one timing slot holds them; `rocprofv3 --kernel-trace --stats -- "
                    "python scripts/crack_skeleton_probe.py` names each).\n")
        f.write("\n## Kernel resources (`scripts/kernel_notes.py k_cs_`, gfx950)\n\n```\n" + notes + "```\n")
        f.write("\n## The timed step\n\n")
        if BENCH_NOTE:
            f.write("`" + BENCH_CMD + "` in the same session: " + BENCH_NOTE + ".  `bench.py` calls none of the new entry points.\n")
        else:
            f.write("This tree against the parent commit, alternating in one session: not measured.  The command, in each tree in "
                    "turn: `" + BENCH_CMD + "`.  `bench.py` calls none of the new entry points.\n")
    print(open(OUT).read())


if __name__ == "__main__":
    main()
