#!/usr/bin/env python3
"""Crack lengths on the map (pcp_crack_lengths) on one MI355X; writes profiles/crack_length_probe.md.  Not collected by pytest.

  The scene of scripts/crack_fuse_probe.py: a noisy tilted wall of POINTS map points (default 10 M) seen at 1920 x 1080 by
  FRAMES keyframes (default 256) around the identity pose, thin-crack masks; ADDED of the keyframes (default 16) are added.
    components wall time and kernel time of pcp_crack_components (min_views 1, radius 0.02) on that state;
    lengths    the same for pcp_crack_lengths, which runs the component stage first: the difference is the stage's own;
    rounds     relaxation rounds of the two sweeps together: every round is one timed launch, so it is the number of timed
               launches of the call minus those of the component stage and the stage's 8 other brackets;
    fetch      wall time of the table and path fetches
  At fewer than 10 M points the file says so in its first paragraph: the figures are then those of the smaller scene.
  The split of the stage's kernel time into k_cl_relax and the others needs the kernels' names: pass the .csv of
  `rocprofv3 --kernel-trace --stats -- python scripts/crack_length_probe.py ...` as the sixth argument of a second run, or
  leave it out (the file then says so).
  resources    scripts/kernel_notes.py k_cl_

  The measurements can be kept apart from the file: with a seventh argument the run saves them there as JSON, or, if that
  file exists, renders the file from it without touching a GPU (the kernel stats and the bench figures of the same session
  come in only after the run that measures).

    python scripts/crack_length_probe.py [points] [frames] [added] [the bench figures to quote, or ""] [output file] [kernel stats csv]
                                         [measurements json]
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
import _crack_width_ref as ref  # noqa: E402
import _mask_edt_ref as edt_ref  # noqa: E402
from pointcloudprocessor_amd import capi  # noqa: E402

POINTS = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 256
ADDED = int(sys.argv[3]) if len(sys.argv) > 3 else 16
BENCH_NOTE = sys.argv[4] if len(sys.argv) > 4 else ""
OUT = sys.argv[5] if len(sys.argv) > 5 and sys.argv[5] else os.path.join(ROOT, "profiles", "crack_length_probe.md")
STATS = sys.argv[6] if len(sys.argv) > 6 else ""
KEEP = sys.argv[7] if len(sys.argv) > 7 else ""
W, H = 1920, 1080
OTHER_BRACKETS = 8  # rows; seed and ends of each sweep (4); the end after sweep 1; pred, count and scan; fill and positions
BENCH_CMD = "python bench.py --gpus 1 --steps 20 --warmup 3 --no-side-legs --no-cpu --no-ic-leg"


def timed(ctx, fn):
    """(kernel ms per slot, launches per slot, wall ms, result) of one call"""
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    got = [ctx.timing_get(k) for k in range(capi.K_COUNT)]
    ctx.timing_enable(False)
    return np.array([g[0] for g in got]), np.array([g[1] for g in got]), wall, out


def kernel_split(path):
    """name -> (calls, total ms, shortest ms, longest ms) of the k_cl_ kernels in a rocprofv3 kernel stats csv"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "k_cl_" in name:
                out[name.split("(")[0].replace("void ", "")] = (int(row["Calls"]), float(row["TotalDurationNs"]) / 1e6, float(row["MinNs"]) / 1e6,
                                                                      float(row["MaxNs"]) / 1e6)
    return out


def measure():
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
        ctx.crack_fuse_begin()
        for f in added:
            ctx.crack_fuse_add(f)
        ctx.crack_components(1, 0.02)  # warm-up: allocates the grid
        ms_c, n_c, wall_c, comp = timed(ctx, lambda: ctx.crack_components(1, 0.02))
        prm = capi.CrackLinkParams(1, 0.02)
        pos = np.empty(len(cloud), np.uint64)
        cracks, entries = capi.C.c_int64(), capi.C.c_int64()

        def call():
            ctx._check(ctx.lib.pcp_crack_lengths(ctx.h, capi.C.byref(prm), capi._ptr(pos), capi.C.byref(cracks), capi.C.byref(entries)))

        ms_l, n_l, wall_l, _ = timed(ctx, call)  # the one call of the stage in a run of this script
        t0 = time.perf_counter()
        c, e = cracks.value, entries.value
        ids, rows, offsets, path = np.empty(c, np.int32), np.empty((c, 7), np.int64), np.zeros(c + 1, np.int64), np.empty(e, np.int32)
        got = capi.C.c_int64()
        ctx._check(ctx.lib.pcp_crack_lengths_fetch(ctx.h, capi.C.c_int64(0), capi.C.c_int64(c), capi._ptr(ids), capi._ptr(rows), capi._ptr(offsets),
                                                   capi.C.byref(got)))
        ctx._check(ctx.lib.pcp_crack_paths_fetch(ctx.h, capi.C.c_int64(0), capi.C.c_int64(e), capi._ptr(path), capi.C.byref(got)))
        wall_fetch = (time.perf_counter() - t0) * 1e3
        ctx.crack_fuse_end()
    longest = int(np.argmax(rows[:, 2])) if len(rows) else -1
    return dict(points=len(cloud), frames=FRAMES, added=len(added), crack_points=int(comp["crack_points"]), cracks=int(comp["components"]),
                wall_c=wall_c, kernels_c=float(ms_c.sum()), wall_l=wall_l, kernels_l=float(ms_l.sum()),
                rounds=int(n_l[capi.K_MISC] - n_c[capi.K_MISC] - OTHER_BRACKETS), wall_fetch=wall_fetch, path_points=e,
                longest=[int(ids[longest]), float(rows[longest, 2] * 2.0 ** -20), int(rows[longest, 3])] if longest >= 0 else None)


def main():
    if KEEP and os.path.exists(KEEP):
        with open(KEEP) as f:
            m = json.load(f)
    else:
        m = measure()
        if KEEP:
            with open(KEEP, "w") as f:
                json.dump(m, f)
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_cl_"], capture_output=True, text=True).stdout
    own_wall, own_kernels = m["wall_l"] - m["wall_c"], m["kernels_l"] - m["kernels_c"]
    with open(OUT, "w") as f:
        f.write("# Crack lengths on the map: measurements (`scripts/crack_length_probe.py`, one MI355X)\n\n")
        f.write(f"The scene of `crack_fuse_probe.py`: a noisy tilted wall of {m['points']} map points at 2-4 m, {W} x {H}, {m['frames']} keyframes "
                f"within 5 cm of the identity pose, z-buffer cull, thin-crack masks; {m['added']} keyframes added.  Kernel times are hipEvent "
                "times of one call's launches (every timing slot, timing on), wall times include the call's synchronisation and, for "
                "`pcp_crack_lengths`, one 4-byte read per round.\n\n")
        if m["points"] < 9_000_000:
            f.write(f"**This is not the 10 M-point scene.**  It was measured at {m['points']} points, where the masks make {m['crack_points']} crack "
                    "points with some 140 links each; at 10 M points they make 3.6 M crack points with five times the links each, so a round "
                    "costs some 25 times what it costs here: a call there is estimated at a quarter of an hour and was not run.  The "
                    "10 M-point figures are not measured.\n\n")
        f.write("| what | figure |\n|---|---|\n")
        f.write("| `pcp_crack_components` (min_views 1, radius 0.02): %d crack points, %d cracks: wall; kernels | %.3f ms; %.3f ms |\n"
                % (m["crack_points"], m["cracks"], m["wall_c"], m["kernels_c"]))
        f.write("| `pcp_crack_lengths` on the same state, positions downloaded (it runs the component stage first): wall; kernels | %.3f ms; %.3f ms |\n"
                % (m["wall_l"], m["kernels_l"]))
        f.write("| the stage's own share (the difference): wall; kernels | %.3f ms; %.3f ms |\n" % (own_wall, own_kernels))
        f.write("| relaxation rounds, both sweeps together (timed launches of the call minus the component stage's and %d others) | %d |\n"
                % (OTHER_BRACKETS, m["rounds"]))
        f.write("| per round: the stage's own wall share over the rounds; of it outside the kernels (launch, the 4-byte read, the "
                "synchronisation) | %.3f ms; %.3f ms |\n" % (own_wall / max(m["rounds"], 1), (own_wall - own_kernels) / max(m["rounds"], 1)))
        f.write("| `pcp_crack_lengths_fetch` of every row and `pcp_crack_paths_fetch` of every entry: wall | %.3f ms |\n" % m["wall_fetch"])
        f.write("| path entries over all cracks; the longest crack: id, length, hops | %d; %s |\n"
                % (m["path_points"], "%d, %.4f m, %d" % tuple(m["longest"]) if m["longest"] else "none"))
        if STATS:
            split = kernel_split(STATS)
            f.write("\n## The stage's kernels (`rocprofv3 --kernel-trace --stats` over another run of this script in the same session: one call "
                    "of the stage, after two of `pcp_crack_components`)\n\n")
            f.write("| kernel | calls | total ms | shortest ms | longest ms |\n|---|---|---|---|---|\n")
            for name, (calls, ms, lo, hi) in sorted(split.items(), key=lambda kv: -kv[1][1]):
                f.write("| `%s` | %d | %.3f | %.3f | %.3f |\n" % (name, calls, ms, lo, hi))
            f.write("\n`k_cl_pred` is one pass of every crack point over all its links, weights included: a round of `k_cl_relax` that costs "
                    "as much has every crack point active.  The plain round schedule of CL8 keeps a point active as long as improvements of "
                    "single units keep arriving from upstream.\n")
        else:
            f.write("| the stage's kernel time split into `k_cl_relax` and the others | not measured: one timing slot holds them; "
                    "`rocprofv3 --kernel-trace --stats -- python scripts/crack_length_probe.py` names each |\n")
        f.write("\n## Kernel resources (`scripts/kernel_notes.py k_cl_`, gfx950)\n\n```\n" + notes + "```\n")
        f.write("\n## The timed step\n\n")
        if BENCH_NOTE:
            f.write("`" + BENCH_CMD + "` in the same session: " + BENCH_NOTE + ".  `bench.py` calls none of the new entry points.\n")
        else:
            f.write("This tree against the parent commit, alternating in one session: not measured.  The command, in each tree in "
                    "turn: `" + BENCH_CMD + "`.  `bench.py` calls none of the new entry points.\n")
    print(open(OUT).read())


if __name__ == "__main__":
    main()
