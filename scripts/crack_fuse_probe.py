#!/usr/bin/env python3
"""Crack widths on the map (pcp_crack_fuse_*, pcp_crack_components) on one MI355X; writes profiles/crack_fuse_probe.md.  Not
collected by pytest.

  C3-like input: a noisy tilted wall of POINTS map points (default 10 M) seen at 1920 x 1080 by FRAMES keyframes (default 256)
  around the identity pose, thin-crack masks (tests/_mask_edt_ref.py); ADDED of the keyframes (default 16) get a mask and are
  added, which is what the per-keyframe figures need.
    add        hipEvent time of one pcp_crack_fuse_add's launches (every timing slot) and its wall time, mean over the adds;
    width      the same for pcp_crack_width with the flag and width images downloaded, and its wall time with every output NULL;
    gather     add's kernel time minus width's: k_cf_gather (the only launch the add has on top);
    components wall time of pcp_crack_components and its kernel time, the grid's slot (PCP_K_MLS_GRID) apart from the rest
               (flag, compaction, gather, union, flatten, ranks, table: PCP_K_MISC);
    fetch      wall time of pcp_crack_fuse_fetch with all nine arrays
  resources    scripts/kernel_notes.py k_cf_ k_cc_

    python scripts/crack_fuse_probe.py [points] [frames] [added] [the plain bench figures to quote, or ""] [output file]
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _crack_width_ref as ref  # noqa: E402
import _mask_edt_ref as edt_ref  # noqa: E402
from pointcloudprocessor_amd import capi  # noqa: E402

POINTS = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 256
ADDED = int(sys.argv[3]) if len(sys.argv) > 3 else 16
BENCH_NOTE = sys.argv[4] if len(sys.argv) > 4 else ""
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "crack_fuse_probe.md")
W, H = 1920, 1080
BENCH_CMD = "python bench.py --gpus 1 --steps 20 --warmup 3 --no-side-legs --no-cpu --no-ic-leg"


def slots(ctx):
    return np.array([ctx.timing_get(k)[0] for k in range(capi.K_COUNT)])


def timed(ctx, fn):
    """(kernel ms per slot, wall ms) of one call"""
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    ms = slots(ctx)
    ctx.timing_enable(False)
    return ms, wall, out


def main():
    shape = (H, W)
    rng = np.random.default_rng(1)
    with capi.Context(0) as ctx:
        ctx.set_camera(capi.camera_from_dict(ref.camera(shape)), capi.default_cull_params())
        _, c2w = capi.pose_to_matrices(ref.IDENTITY_POSE)
        cloud = ref.wall_cloud(shape, seed=1, density=POINTS / (H * W), c2w=c2w)
        ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
        poses = np.tile(ref.IDENTITY_POSE, (FRAMES, 1))
        poses[:, :3] = rng.uniform(-0.05, 0.05, (FRAMES, 3))
        ctx.set_frames(poses)
        added = list(range(min(ADDED, FRAMES)))
        for f in added:
            ctx.upload_mask(f, edt_ref.crack_mask(shape, seed=100 + f, cracks=8))
        ctx.crack_width(0, want=("flags", "width"))  # warm-up: allocates
        k_w, wall_w, bare_w = [], [], []
        for f in added:
            ms, wall, _ = timed(ctx, lambda: ctx.crack_width(f, want=("flags", "width")))
            k_w.append(ms.sum())
            wall_w.append(wall)
            bare_w.append(timed(ctx, lambda: ctx.crack_width(f, want=()))[1])
        ctx.crack_fuse_begin()
        k_a, wall_a, credited = [], [], 0
        for f in added:
            ms, wall, (m, c) = timed(ctx, lambda: ctx.crack_fuse_add(f))
            k_a.append(ms.sum())
            wall_a.append(wall)
            credited += c
        ms_c, wall_c, comp = timed(ctx, lambda: ctx.crack_components(1, 0.02))
        _, wall_f, _ = timed(ctx, ctx.crack_fuse_fetch)
        ctx.crack_fuse_end()
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_cf_", "k_cc_"], capture_output=True, text=True).stdout
    with open(OUT, "w") as f:
        f.write("# Crack widths on the map: measurements (`scripts/crack_fuse_probe.py`, one MI355X)\n\n")
        f.write(f"A noisy tilted wall of {len(cloud)} map points at 2-4 m, {W} x {H}, {FRAMES} keyframes within 5 cm of the identity pose, "
                f"z-buffer cull, thin-crack masks; {len(added)} keyframes added.  Kernel times are hipEvent times of one call's launches "
                "(every timing slot), wall times include the call's synchronisation; means over the added keyframes.\n\n")
        f.write("| what | figure |\n|---|---|\n")
        f.write("| `pcp_crack_fuse_add`: kernels / wall | %.3f ms / %.3f ms |\n" % (np.mean(k_a), np.mean(wall_a)))
        f.write("| `pcp_crack_width`, flags and width downloaded: kernels / wall; wall with every output NULL | %.3f ms / %.3f ms; %.3f ms |\n"
                % (np.mean(k_w), np.mean(wall_w), np.mean(bare_w)))
        f.write("| `k_cf_gather` per keyframe (add's kernels minus the width call's) | %.3f ms |\n" % (np.mean(k_a) - np.mean(k_w)))
        f.write("| a second width stage per keyframe when `--crackWidth 1` and `--crackFuse 1` are both given | the `pcp_crack_width` line |\n")
        f.write("| credited samples over the added keyframes | %d |\n" % credited)
        f.write("| `pcp_crack_components` (min_views 1, radius 0.02): %d crack points, %d cracks: wall; grid kernels; the other kernels | "
                "%.3f ms; %.3f ms; %.3f ms |\n" % (comp["crack_points"], comp["components"], wall_c, ms_c[capi.K_MLS_GRID], ms_c.sum() - ms_c[capi.K_MLS_GRID]))
        f.write("| the other kernels split into union, flatten and table | not measured: one timing slot holds them; "
                "`rocprofv3 --kernel-trace --stats -- python scripts/crack_fuse_probe.py` names each |\n")
        f.write("| `pcp_crack_fuse_fetch`, nine arrays (40 B per point) to pageable memory: wall | %.3f ms |\n" % wall_f)
        f.write("\n## Kernel resources (`scripts/kernel_notes.py k_cf_ k_cc_`, gfx950)\n\n```\n" + notes + "```\n")
        f.write("\n## The timed step\n\n")
        if BENCH_NOTE:
            f.write("`" + BENCH_CMD + "` in the same session: " + BENCH_NOTE + ".  `bench.py` calls none of the new entry points.\n")
        else:
            f.write("This tree against the parent commit, alternating in one session: not measured.  The command, in each tree in "
                    "turn: `" + BENCH_CMD + "`.  `bench.py` calls none of the new entry points.\n")
    print(open(OUT).read())


if __name__ == "__main__":
    main()
