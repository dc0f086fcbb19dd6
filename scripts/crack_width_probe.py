#!/usr/bin/env python3
"""Crack width maps (pcp_crack_width) on one MI355X; writes profiles/crack_width_probe.md.  Not collected by pytest.

  per size (1920x1080, 4096x3000) and mask (thin cracks, synth.make_mask discs, one background pixel in a corner), over a
  noisy tilted wall with about 0.3 points per pixel (tests/_crack_width_ref.py):
    kernels    hipEvent time of one call's launches (PCP_K_MISC and the cull's slots, pcp_timing_*): the geometry scatter, the
               distance transform, the tables and the site kernel; steady state, mean of the timed calls after a warm-up;
    maps       the same for pcp_frame_geometry + pcp_mask_edt alone (what the call runs first), so the difference is the
               call's own five kernels;
    bare       wall time of the call without any download (every output NULL);
    call       wall time with flags, edges, w2d2, width, points and plane downloaded
  resources    scripts/kernel_notes.py k_cw_

    python scripts/crack_width_probe.py [the plain bench figures to quote, or ""] [output file]
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
from pointcloudprocessor_amd import capi, synth  # noqa: E402

BENCH_NOTE = sys.argv[1] if len(sys.argv) > 1 else ""
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "crack_width_probe.md")
SIZES = [(1920, 1080), (4096, 3000)]
REPS = 5
BENCH_CMD = "python bench.py --gpus 1 --steps 20 --warmup 3 --no-side-legs --no-cpu --no-ic-leg"


def masks_of(w, h):
    return [("thin cracks", edt_ref.crack_mask((h, w), seed=1, cracks=8)), ("discs", synth.make_mask(0, w, h)),
            ("one background pixel", edt_ref.corner_mask((h, w)))]


def timed(ctx, fn, reps):
    """(kernel ms over every slot, median wall ms) of `reps` steady-state calls"""
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    ms = sum(ctx.timing_get(k)[0] for k in range(capi.K_COUNT)) / reps
    ctx.timing_enable(False)
    return ms, float(np.median(wall))


def main():
    rows = []
    for w, h in SIZES:
        shape = (h, w)
        with capi.Context(0) as ctx:
            cull = capi.default_cull_params()
            ctx.set_camera(capi.camera_from_dict(ref.camera(shape)), cull)
            _, c2w = capi.pose_to_matrices(ref.IDENTITY_POSE)
            cloud = ref.wall_cloud(shape, seed=1, c2w=c2w)
            ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
            ctx.set_frames(np.tile(ref.IDENTITY_POSE, (2, 1)))
            for name, mask in masks_of(w, h):
                ctx.upload_mask(0, mask)
                out = ctx.crack_width(0)  # warm-up: allocates
                k_all, call = timed(ctx, lambda: ctx.crack_width(0), REPS)
                _, bare = timed(ctx, lambda: ctx.crack_width(0, want=()), REPS)

                def maps_only():
                    ctx.lib.pcp_frame_geometry(ctx.h, 0, None, None, None, None, None)
                    ctx.lib.pcp_mask_edt(ctx.h, 0, 0, None, None)

                k_maps, _ = timed(ctx, maps_only, REPS)
                wd = out["width"][(out["flags"] & capi.CW_WIDTH) != 0]
                rows.append((f"{w}x{h}", name, len(cloud), out["sites"], out["widths"], float(np.median(wd)) * 1e3 if len(wd) else 0.0,
                             k_all, k_maps, k_all - k_maps, bare, call))
                print(rows[-1], flush=True)
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_cw_"], capture_output=True, text=True).stdout
    with open(OUT, "w") as f:
        f.write("# Crack width maps: measurements (`scripts/crack_width_probe.py`, one MI355X)\n\n")
        f.write("A noisy tilted wall at 2-4 m with about 0.3 points per pixel, identity pose, z-buffer cull.  Kernel times are hipEvent "
                "times of one call's launches (every timing slot: the cull of `pcp_frame_visible`, the geometry scatter, the distance "
                "transform and the call's own kernels under `PCP_K_MISC`), the mean of %d steady-state calls after a warm-up.  `maps` "
                "is the same for `pcp_frame_geometry` + `pcp_mask_edt` alone without downloads (what the call runs first), `own` the "
                "difference: the tables and the site kernel.  `bare` is the wall time of the call with every output NULL, `call` "
                "with flags, edges, w2d2, width, points and plane downloaded to pageable host memory (73 B per pixel).\n\n" % REPS)
        f.write("| image | mask | points | sites | widths | median width mm | kernels ms | maps ms | own ms | bare ms | call ms |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %s | %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.2f | %.2f |\n" % r)
        f.write("\n## Kernel resources (`scripts/kernel_notes.py k_cw_`, gfx950)\n\n```\n" + notes + "```\n")
        f.write("\n## The timed step\n\n")
        if BENCH_NOTE:
            f.write("`" + BENCH_CMD + "` in the same session: " + BENCH_NOTE + ".  `bench.py` calls none of the new entry points.\n")
        else:
            f.write("This tree against the parent commit, alternating in one session: not measured.  The command, in each tree in "
                    "turn: `" + BENCH_CMD + "`.  `bench.py` calls none of the new entry points.\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
