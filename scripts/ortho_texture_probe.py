#!/usr/bin/env python3
"""The orthophoto ("Orthophotos") at scale, on one MI355X.  Run it under one `timeout`.

    python scripts/ortho_texture_probe.py [--points N] [--frames F] [--gsd G] [--scale K] [--views M] [--repeats 3]

The C3 shape: 10 M points x 256 keyframes at 1920x1080, coloured in one shot (the colour pass's device time of the same session
is printed beside the orthophoto's as context); the coloured rows' map in the auto frame at 5 mm, filled at R = 4; the orthophoto
at k = 5 over the whole raster: device time of its kernel (PCP_K_MISC), the visits (surface pixels x keyframes walked) per second,
the share of (tile, keyframe) pairs the tile test skipped.  Two warm-up rounds, then --repeats rounds; median [min .. max].
PCP_HIP_LIBRARY selects another build of the same ABI: how the plain loop (profiles/ortho_texture_plain_loop.patch) is measured
against the tile lists.  One JSON line per measurement on stdout, progress on stderr.  Not collected by pytest."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--gsd", type=float, default=0.005)
    ap.add_argument("--scale", type=int, default=5)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import numpy as np

    from pointcloudprocessor_amd import capi, synth

    def say(**kw):
        print(json.dumps(kw), flush=True)

    say(library=os.environ.get("PCP_HIP_LIBRARY", "default"), points=args.points, frames=args.frames, gsd=args.gsd, scale=args.scale)
    x, y, z, _ = synth.make_cloud(args.points, seed=synth.SEED)
    xyz = np.stack([x, y, z], axis=1)
    cd = synth.camera_dict("cfg")
    W, H = cd["image_width"], cd["image_height"]
    poses, _ = synth.make_trajectory(args.frames, seed=synth.SEED)
    with capi.Context(0) as ctx:
        ctx.set_camera(capi.camera_from_dict(cd))
        e = x[:0]
        ctx.upload_cloud(e, e, e)  # (the image uploads ask for a cloud)
        ctx.set_frames(poses)
        for f in range(args.frames):
            ctx.upload_image(f, synth.make_image(f, W, H))
        ctx.synchronize()
        print("images uploaded", file=sys.stderr, flush=True)
        ctx.timing_enable(True)
        ctx.upload_cloud(x, y, z)
        colour = []
        for rep in range(2 + args.repeats):
            ctx.synchronize()
            ctx.timing_reset()
            ctx.colorize(download=False)
            ctx.synchronize()
            if rep >= 2:
                colour.append(sum(ctx.timing_get(k)[0] for k in (capi.K_TILE_MASK, capi.K_DEPTH, capi.K_COLOUR)))
        has = (ctx.download_result_packed() >> 24).astype(np.uint8)
        say(case="colour pass (tile masks + depth + colour), device ms", coloured=int(has.sum()), ms=spread(colour))
        frame = capi.ortho_fit_frame_host(xyz, args.gsd, has=has, viewer=np.asarray(poses, np.float64).reshape(-1, 7)[:, :3].mean(axis=0))
        ctx.ortho_begin(frame)
        ctx.ortho_add(0)
        occupied, filled = ctx.ortho_finish(4)
        p = capi.ortho_texture_params(args.scale, args.views, True, 0.05)
        fh, fw = frame.height * args.scale, frame.width * args.scale
        counts = np.zeros(4, np.int64)
        dev, wall = [], []
        for rep in range(2 + args.repeats):  # no layer leaves the device in the timed rounds: the kernel alone
            ctx.synchronize()
            ctx.timing_reset()
            t0 = time.perf_counter()
            ctx._check(ctx.lib.pcp_ortho_texture(ctx.h, capi.C.byref(p), None, None, None, None, None, capi._ptr(counts)))
            wall_ms = (time.perf_counter() - t0) * 1e3
            if rep >= 2:
                dev.append(ctx.timing_get(capi.K_MISC)[0])
                wall.append(wall_ms)
        surface, textured, unseen, skipped = (int(v) for v in counts)
        t0 = time.perf_counter()
        out = ctx.ortho_texture(args.scale, args.views, True, 0.05)
        full_wall = (time.perf_counter() - t0) * 1e3
        assert (out["surface"], out["textured"], out["unseen"], out["skipped_pairs"]) == (surface, textured, unseen, skipped)
        # the pairs of the tiles that hold a surface point: every such tile either walks or skips each keyframe
        st = out["status"]
        th, tw = -(-fh // 16), -(-fw // 16)
        pad = np.zeros((th * 16, tw * 16), bool)
        pad[:fh, :fw] = st > 0
        tiles = int(pad.reshape(th, 16, tw, 16).any(axis=(1, 3)).sum())
        pairs = tiles * args.frames
        walked = pairs - skipped
        ms = statistics.median(dev)
        say(case="orthophoto", raster=[frame.width, frame.height], fine=[fw, fh], occupied=occupied, filled_r4=filled, surface=surface,
            textured=textured, unseen=unseen, tiles_with_surface=tiles, pairs=pairs, skipped_pairs=skipped,
            skipped_share=round(skipped / max(pairs, 1), 4), kernel_ms=spread(dev), call_wall_ms_no_layers=spread(wall),
            call_wall_ms_all_layers=round(full_wall, 1), lane_visits=walked * 256, lane_visits_per_second=round(walked * 256 / (ms * 1e-3), 0),
            views_histogram=np.bincount(np.minimum(out["count"][st > 0], 8), minlength=9).tolist(),
            rgb_checksum=int(np.frombuffer(out["rgb"].tobytes(), np.uint8).astype(np.uint64).sum()))
        ctx.ortho_end()


if __name__ == "__main__":
    main()
