#!/usr/bin/env python3
"""Cost of PCP_MATCH_RADIUS against PCP_MATCH_ROUNDTRIP on the bench's C3 map (10 M points x 256 keyframes at 1920x1080).

    python scripts/match_radius_probe.py [--points N] [--frames F] [--steps K] [--dup 0.01]

A step is pcp_colorize without a download (depth pass + colour pass, plus the fix-up in RADIUS mode).  The two modes
alternate in one process, one context each, ROUNDTRIP first, over --rounds rounds of --steps steps; ms_per_step is the
median of the rounds.  Then --dup of the points are copied (half exact copies, half 4 um away) and the same is measured on
that map, with the table build (first RADIUS call after pcp_upload_cloud, minus a steady RADIUS step).  One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def steps_ms(ctx, k):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        ctx.colorize(download=False)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / k


def measure(ctxs, steps, rounds):
    """ctxs: mode -> a context holding the same map and keyframes, configured for that mode"""
    out = {m: [] for m in ctxs}
    for ctx in ctxs.values():  # warm-up (and the table build)
        steps_ms(ctx, 3)
    for _ in range(rounds):
        for m, ctx in ctxs.items():
            out[m].append(steps_ms(ctx, steps))
    return {m: float(np.median(v)) for m, v in out.items()}, out


def load(ctx, capi, synth, cd, mode, x, y, z, poses):
    ctx.set_camera(capi.camera_from_dict(cd), cull(capi, mode))
    ctx.upload_cloud(x, y, z)
    ctx.set_frames(poses)
    for f in range(len(poses)):
        ctx.upload_image(f, synth.make_image(f, cd["image_width"], cd["image_height"]))
    ctx.synchronize()


def cull(capi, mode):
    cp = capi.default_cull_params()
    cp.match_mode = capi.MATCH_RADIUS if mode == "radius" else capi.MATCH_ROUNDTRIP
    return cp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dup", type=float, default=0.01)
    args = ap.parse_args()
    from pointcloudprocessor_amd import capi, synth

    cd = synth.camera_dict("cfg")
    x, y, z, _ = synth.make_cloud(args.points, seed=synth.SEED)
    poses, _ = synth.make_trajectory(args.frames, seed=synth.SEED)
    res = dict(points=args.points, frames=args.frames, camera="cfg 1920x1080", steps=args.steps, rounds=args.rounds)
    # one context per mode (pcp_set_camera drops the images): the same map, keyframes and images in both
    with capi.Context(0) as rt, capi.Context(0) as rd:
        for ctx, mode in ((rt, "roundtrip"), (rd, "radius")):
            load(ctx, capi, synth, cd, mode, x, y, z, poses)
        med, raw = measure({"roundtrip": rt, "radius": rd}, args.steps, args.rounds)
        res["ms_per_step"] = med
        res["ms_per_step_rounds"] = raw
        res["radius_over_roundtrip"] = med["radius"] / med["roundtrip"]
        # the duplicated map: --dup of the points copied, half exactly, half 4 um away
        rng = np.random.default_rng(3)
        m = int(args.points * args.dup)
        pick = rng.choice(len(x), m, replace=False)
        off = (rng.normal(0, 1, (m, 3)) * 4e-6 / np.sqrt(3)).astype(np.float32)
        off[: m // 2] = 0.0
        xd = np.concatenate([x, x[pick] + off[:, 0]]).astype(np.float32)
        yd = np.concatenate([y, y[pick] + off[:, 1]]).astype(np.float32)
        zd = np.concatenate([z, z[pick] + off[:, 2]]).astype(np.float32)
        for ctx in (rt, rd):
            ctx.upload_cloud(xd, yd, zd)  # (keyframes and images stay)
            ctx.synchronize()
        t0 = time.perf_counter()
        rd.colorize(download=False)  # builds the table
        rd.synchronize()
        first = (time.perf_counter() - t0) * 1e3
        steady = steps_ms(rd, args.steps)
        res["dup"] = dict(copies=m, close_pairs_2_5e_5=int(rd.close_pairs(2.5e-5)), first_radius_call_ms=first,
                          steady_radius_ms=steady, table_build_ms=first - steady)
        med_d, raw_d = measure({"roundtrip": rt, "radius": rd}, args.steps, args.rounds)
        res["dup"]["ms_per_step"] = med_d
        res["dup"]["ms_per_step_rounds"] = raw_d
        res["dup"]["fixup_ms_estimate"] = med_d["radius"] - med_d["roundtrip"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
