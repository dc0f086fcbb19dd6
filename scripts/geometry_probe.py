#!/usr/bin/env python3
"""Geometry maps on the C3 synthetic map (10 M points, 256 keyframes at 1920x1080); one JSON line per measurement.  Not
collected by pytest.

  normals     pcp_estimate_normals at each radius: wall time of the call (median of the timed calls after a warm-up), the
              kernel time of that (PCP_K_MISC: records, work items, compaction, the moments-and-solve kernel; PCP_K_MLS_GRID:
              the grid), the neighbour pairs (sum of the reported counts) and pairs per second of kernel time.  The
              yardstick is the local colour smoothing at the same radius in the same session (pcp_colour_smooth_local_packed:
              the same search, lighter arithmetic; PCP_K_COLOUR_SMOOTH + the grid): the ratio of the two kernel times.
  maps        pcp_frame_geometry over the first keyframes: wall time per keyframe with all four images downloaded, with no
              output (the normals are then not resolved), and the kernel time of the downloading form (depth, visibility,
              compaction, clear / scatter / resolve).
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudprocessor_amd import capi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 256
RADII = [float(v) for v in sys.argv[3:]] or [0.03, 0.1]
MAP_FRAMES = 16
KERNELS = (capi.K_MISC, capi.K_MLS_GRID, capi.K_COLOUR_SMOOTH, capi.K_DEPTH, capi.K_VISIBILITY, capi.K_PROJECT)


def timed(ctx, fn, reps):
    """(wall ms per call, {kernel id: ms per call}) over reps calls"""
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    ms = {k: ctx.timing_get(k)[0] / reps for k in KERNELS}
    ctx.timing_enable(False)
    return wall, ms


def main():
    x, y, z, _ = synth.make_cloud(N)
    cd = synth.camera_dict("cfg")
    poses, _ = synth.make_trajectory(FRAMES)
    words = np.random.default_rng(1).integers(0, 1 << 25, N, dtype=np.uint32)
    with capi.Context(0) as ctx:
        ctx.set_camera(capi.camera_from_dict(cd))
        ctx.upload_cloud(x, y, z)
        ctx.set_frames(poses)
        for r in RADII:
            valid = ctx.estimate_normals(r)  # warm-up
            pairs = int(ctx.normals_fetch()["neighbours"].astype(np.int64).sum())
            wall, ms = timed(ctx, lambda: ctx.estimate_normals(r), 5)
            ctx.colour_smooth_local_packed(r, words)  # warm-up
            swall, sms = timed(ctx, lambda: ctx.colour_smooth_local_packed(r, words), 5)
            k_normals = ms[capi.K_MISC] + ms[capi.K_MLS_GRID]
            k_smooth = sms[capi.K_COLOUR_SMOOTH] + sms[capi.K_MLS_GRID]
            print(json.dumps({
                "what": "normals", "n": N, "radius": r, "valid": valid, "pairs": pairs, "neighbours_mean": round(pairs / N, 1),
                "call_ms_median": round(float(np.median(wall)), 3), "kernel_ms": round(k_normals, 3),
                "of_which_grid_ms": round(ms[capi.K_MLS_GRID], 3), "pairs_per_s": round(pairs / (k_normals * 1e-3), 0),
                "smooth_call_ms_median": round(float(np.median(swall)), 3), "smooth_kernel_ms": round(k_smooth, 3),
                "smooth_misc_ms": round(sms[capi.K_MISC], 3), "normals_over_smooth": round(k_normals / k_smooth, 3),
            }), flush=True)
        frames = list(range(min(MAP_FRAMES, FRAMES)))
        ctx.frame_geometry(0)  # warm-up: allocates the images
        it = iter(frames * 2)
        occupied = [ctx.frame_geometry(f)["pixels"] for f in frames]
        wall, ms = timed(ctx, lambda: ctx.frame_geometry(next(it)), len(frames))
        it = iter(frames)
        px = C.c_int64()
        bare, _ = timed(ctx, lambda: ctx._check(ctx.lib.pcp_frame_geometry(ctx.h, C.c_int32(next(it)), None, None, None, None, C.byref(px))),
                        len(frames))
        hh, ww = cd["image_height"], cd["image_width"]
        print(json.dumps({
            "what": "maps", "n": N, "keyframes": len(frames), "image": [ww, hh], "download_mb": round(hh * ww * 32 / 1e6, 1),
            "occupied_px_mean": int(np.mean(occupied)), "with_download_ms_median": round(float(np.median(wall)), 3),
            "no_output_ms_median": round(float(np.median(bare)), 3),
            "kernel_ms": {"depth": round(ms[capi.K_DEPTH], 3), "visibility": round(ms[capi.K_VISIBILITY], 3), "misc": round(ms[capi.K_MISC], 3)},
        }), flush=True)


if __name__ == "__main__":
    main()
