#!/usr/bin/env python3
"""Cost of the exposure gains (pcp_view_pair_stats, pcp_exposure_gains, the gained finalise); writes one JSON file.  Not
collected by pytest.

    python scripts/exposure_probe.py [out.json] [n_points] [n_frames]

  stats      C3-size state (10 M points x 256 keyframes @1920x1080, synth images scaled per keyframe): pcp_view_pair_stats
             REPS times -- the PCP_K_MISC kernel time (device events) and the wall time of the call with its two F x F
             downloads --, the cells filled, and what the kernel issued: wavefront partials, 64-bit adds at the flush of the
             workgroups' tables, adds issued directly.  state_read_bytes = the 40 B per point the kernel reads.
  solve      pcp_exposure_gains on the host: the matrices of the run (F keyframes), and synthetic band matrices at F = 2048
  finalise   plain finalise (PCP_K_COLOUR) against the gained finalise (PCP_K_MISC) on the same state, alternating
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudprocessor_amd import capi, synth  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "exposure_probe.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
F = int(sys.argv[3]) if len(sys.argv) > 3 else 256
REPS = 7
K = (0.6, 1.4, 0.8, 1.2, 1.0, 0.7)


def band_matrices(F, half=24, seed=5):
    """every keyframe shares points with its `half` neighbours on either side; consistent means under per-keyframe exposures"""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.6, 1.5, F)
    n = np.zeros((F, F), np.uint64)
    s = np.zeros((F, F), np.uint64)
    for i in range(F):
        for j in range(i + 1, min(F, i + 1 + half)):
            c = int(rng.integers(100, 100000))
            base = rng.uniform(40, 150)
            n[i, j] = n[j, i] = c
            s[i, j] = int(min(247.0, base * k[i]) * c)
            s[j, i] = int(min(247.0, base * k[j]) * c)
    return n, s


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    cd = synth.camera_dict("cfg")
    W, H = cd["image_width"], cd["image_height"]
    x, y, z, _ = synth.make_cloud(N)
    poses, _ = synth.make_trajectory(F)
    res = {"what": "exposure gains: pair statistics kernel, host solve, gained finalise", "points": N, "keyframes": F,
           "image": f"{W}x{H}", "reps": REPS}
    with capi.Context(0) as ctx:
        ctx.set_camera(capi.camera_from_dict(cd))
        ctx.upload_cloud(x, y, z)
        ctx.set_frames(poses)
        for f in range(F):
            im = synth.make_image(f, W, H)
            ctx.upload_image(f, np.clip(im.astype(np.float32) * np.float32(K[f % 6]), 0, 255).astype(np.uint8))
        ctx.colour_reset()
        ctx.depth_pass()
        ctx.colour_pass()
        ctx.synchronize()
        ctx.view_pair_stats()  # warm
        kern, wall = [], []
        for _ in range(REPS):
            ctx.timing_reset()
            ctx.timing_enable(True)
            (n, s), dt = timed(ctx.view_pair_stats)
            kern.append(ctx.timing_get(capi.K_MISC)[0])
            ctx.timing_enable(False)
            wall.append(dt)
        c = ctx.view_pair_stats_counters()
        waves = (N + 63) // 64
        res["stats"] = {
            "kernel_ms_median": round(float(np.median(kern)), 4), "kernel_ms_min": round(float(np.min(kern)), 4),
            "kernel_ms_all": [round(t, 4) for t in kern], "call_wall_ms_median": round(float(np.median(wall)), 3),
            "filled_cells": int((n > 0).sum()), "pairs": int(n.sum()), "counters": c, "wavefronts": waves,
            "partials_per_wavefront": round(c["wave_partials"] / waves, 3),
            "global_adds_per_wavefront": round((c["flush_adds"] + c["direct_adds"]) / waves, 4),
            "state_read_bytes": 40 * N,
            "state_read_GBps_at_median": round(40 * N / (float(np.median(kern)) * 1e-3) / 1e9, 1),
        }
        with open(OUT, "w") as fh:
            json.dump(res, fh, indent=1)
        g, dt = timed(lambda: capi.exposure_gains(n, s))
        solve = {f"F={F}_ms": round(dt, 3), "gain_min": round(float(g.min()), 4), "gain_max": round(float(g.max()), 4),
                 "active": int((g != 1.0).sum())}
        # plain against gained finalise on the same state
        plain, gained = [], []
        for it in range(REPS + 1):
            for on in (False, True):
                ctx.set_frame_gains(g if on else None)
                ctx.synchronize()
                ctx.timing_reset()
                ctx.timing_enable(True)
                ctx.colour_finalise(download=False)
                ctx.synchronize()
                ms = ctx.timing_get(capi.K_MISC if on else capi.K_COLOUR)[0]
                ctx.timing_enable(False)
                if it:
                    (gained if on else plain).append(ms)
        ctx.set_frame_gains(None)
        res["finalise"] = {"plain_kernel_ms_median": round(float(np.median(plain)), 4), "gained_kernel_ms_median": round(float(np.median(gained)), 4),
                           "plain_all": [round(t, 4) for t in plain], "gained_all": [round(t, 4) for t in gained]}
    with open(OUT, "w") as fh:
        json.dump(res, fh, indent=1)
    nb, sb = band_matrices(2048)
    gb, dt = timed(lambda: capi.exposure_gains(nb, sb))
    solve["F=2048_band_ms"] = round(dt, 1)
    solve["F=2048_gain_range"] = [round(float(gb.min()), 4), round(float(gb.max()), 4)]
    res["solve"] = solve
    with open(OUT, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
