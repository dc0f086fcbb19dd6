#!/usr/bin/env python3
"""Mask distance maps (pcp_mask_edt / pcp_mask_edt_frames) on one MI355X against scipy on the same box's host; writes
profiles/crack_maps_probe.md.  Not collected by pytest.

  per size (1920x1080, 4096x3000) and mask (thin cracks, synth.make_mask discs, one background pixel in a corner):
    kernels    hipEvent time of one call's kernels (PCP_K_MISC, pcp_timing_*), steady state, mean of the timed calls;
               the same call at threshold 255, where every pixel is background: the column stage plus the row stage's
               floor (staging, one compare, the stores) -- the difference is the row stage's search;
    call       wall time of the call with both images downloaded;
    scipy      scipy.ndimage.distance_transform_edt(mask > 0) on the host, the call this replaces;
    check      sqrt(d2) == scipy, every pixel
  batched      pcp_mask_edt_frames over 256 keyframes at 1920x1080 (thin cracks), download included
  resources    scripts/kernel_notes.py k_md_

    python scripts/crack_maps_probe.py [frames, default 256] [the plain bench figures to quote, or ""] [output file]
(the notes under the table of profiles/crack_maps_probe.md were added by hand)
"""
import os
import subprocess
import sys
import time

import numpy as np
import scipy.ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mask_edt_ref as ref  # noqa: E402
from pointcloudprocessor_amd import capi, synth  # noqa: E402

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 256
BENCH_NOTE = sys.argv[2] if len(sys.argv) > 2 else ""
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "crack_maps_probe.md")
SIZES = [(1920, 1080), (4096, 3000)]
REPS = 5


def masks_of(w, h):
    return [("thin cracks", ref.crack_mask((h, w), seed=1, cracks=8)), ("discs", synth.make_mask(0, w, h)),
            ("one background pixel", ref.corner_mask((h, w)))]


def kernel_ms(ctx, fn, reps):
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    ms = ctx.timing_get(capi.K_MISC)[0] / reps
    ctx.timing_enable(False)
    return ms, float(np.median(wall))


def main():
    rows = []
    batched = None
    poses, _ = synth.make_trajectory(FRAMES)
    x, y, z, _ = synth.make_cloud(1000)
    for w, h in SIZES:
        cd = dict(synth.camera_dict("cfg"), image_width=w, image_height=h)
        with capi.Context(0) as ctx:
            ctx.set_camera(capi.camera_from_dict(cd))
            ctx.upload_cloud(x, y, z)
            ctx.set_frames(poses[:4] if (w, h) != SIZES[0] else poses)
            for name, mask in masks_of(w, h):
                ctx.upload_mask(0, mask)
                out = ctx.mask_edt(0)  # warm-up: allocates
                t0 = time.perf_counter()
                want = scipy.ndimage.distance_transform_edt(mask > 0)
                scipy_ms = (time.perf_counter() - t0) * 1e3
                exact = bool(np.array_equal(np.sqrt(out["d2"].astype(np.float64)), want))
                k_full, call = kernel_ms(ctx, lambda: ctx.mask_edt(0), REPS)
                k_floor, _ = kernel_ms(ctx, lambda: ctx.mask_edt(0, 255), REPS)
                rows.append((f"{w}x{h}", name, int(out["d2"].max()), k_full, k_floor, k_full - k_floor, call, scipy_ms, exact))
                print(rows[-1], flush=True)
            if (w, h) == SIZES[0]:
                crack = masks_of(w, h)[0][1]
                for f in range(FRAMES):
                    ctx.upload_mask(f, np.roll(crack, 7 * f, axis=1))
                ctx.mask_edt_frames(0, FRAMES)  # warm-up
                k_b, call_b = kernel_ms(ctx, lambda: ctx.mask_edt_frames(0, FRAMES), 2)
                batched = (FRAMES, k_b, call_b, FRAMES * w * h * 8 / 1e9)
                print(batched, flush=True)
    notes = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_notes.py"), "k_md_"], capture_output=True, text=True).stdout
    path = OUT
    with open(path, "w") as f:
        f.write("# Mask distance maps: measurements (`scripts/crack_maps_probe.py`, one MI355X)\n\n")
        f.write("Kernel times are hipEvent times of one call's launches (`PCP_K_MISC`), the mean of %d steady-state calls; "
                "`floor` is the same call at threshold 255 (every pixel background: the column stage plus the row stage's staging, "
                "one compare and the stores), `search` the difference, i.e. what the outward search of the row stage costs on that "
                "mask.  `call` is the wall time with both images downloaded; `scipy` is `scipy.ndimage.distance_transform_edt` on "
                "the same box's host in the same run.\n\n" % REPS)
        f.write("| image | mask | largest d2 | kernels ms | floor ms | search ms | call ms | scipy ms | sqrt(d2) == scipy |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %s | %d | %.3f | %.3f | %.3f | %.2f | %.0f | %s |\n" % r)
        if batched:
            f.write("\n`pcp_mask_edt_frames` over %d keyframes at 1920x1080 (thin cracks): kernels %.1f ms, the call with its download "
                    "of %.1f GB %.0f ms.\n" % (batched[0], batched[1], batched[3], batched[2]))
        f.write("\n## Kernel resources (`scripts/kernel_notes.py k_md_`, gfx950)\n\n```\n" + notes + "```\n`k_md_rows` takes 4 B of dynamic LDS per pixel of a row.\n")
        if BENCH_NOTE:
            f.write("\n## The timed step\n\n`bench.py --gpus 1` in the same session: " + BENCH_NOTE + ".  `bench.py` calls none of the new entry points.\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
