#!/usr/bin/env python3
"""The orthographic maps ("Orthographic maps") at scale, on one MI355X.  Run it under one `timeout`.

    python scripts/ortho_probe.py [--points N] [--frames F] [--stand-in] [--streamed] [--chunk-log2 28] [--repeats 7]

C3 one-shot: the map's colour result (10 M points x 256 keyframes at 1920x1080), auto frame, at gsd 5 mm and 50 mm: add
(scatter + payload), finish without fill and with R = 4, fetch; atomics per contributor from the stats.
--stand-in: no keyframes and no colour pass: the same map with the has bit set on the rows of a box that holds about 4 % of it (fewer than the
6.7 M rows the colour run of that shape leaves), and on every row (more than it leaves), through ortho_add_packed with the words in device memory.
--streamed: the streamed chain at the reference's configuration (as scripts/stream_colour_probe.py sets it up), sweep B with
ortho= on against off, download=False, in one session.
PCP_HIP_LIBRARY selects another build of the same ABI (how the plain scatter was measured against the merged one).
Per stage: two warm-up rounds, then --repeats rounds; the kernels' device time (PCP_K_MISC) and the host's wall clock, median
[min .. max].  One JSON line per measurement on stdout, progress on stderr.  Not collected by pytest."""
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
    ap.add_argument("--stand-in", action="store_true")
    ap.add_argument("--streamed", action="store_true")
    ap.add_argument("--chunk-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch

    from pointcloudprocessor_amd import capi, pipeline, synth

    def say(**kw):
        print(json.dumps(kw), flush=True)

    say(library=os.environ.get("PCP_HIP_LIBRARY", "default"), points=args.points)
    x, y, z, _ = synth.make_cloud(args.points, seed=synth.SEED)
    xyz = np.stack([x, y, z], axis=1)

    def timed(ctx, fn):
        """device ms of the PCP_K_MISC kernels and wall ms of fn()"""
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return ctx.timing_get(capi.K_MISC)[0], wall, out

    def measure(ctx, name, has, add, want_label=False):
        for gsd in (0.005, 0.05):
            frame = capi.ortho_fit_frame_host(xyz, gsd, has=has)
            rows = {k: [] for k in ("add_dev", "add_wall", "finish0_dev", "finish0_wall", "finish4_dev", "finish4_wall", "fetch_wall")}
            for rep in range(2 + args.repeats):
                ctx.ortho_begin(frame)
                a_dev, a_wall, contributors = timed(ctx, add)
                f0_dev, f0_wall, (occupied, _) = timed(ctx, lambda: ctx.ortho_finish(0))
                f4_dev, f4_wall, (_, filled) = timed(ctx, lambda: ctx.ortho_finish(4))
                _, fe_wall, _ = timed(ctx, lambda: ctx.ortho_fetch(want_label=want_label))
                st = ctx.ortho_stats()
                ctx.ortho_end()
                if rep >= 2:
                    for k, v in zip(rows, (a_dev, a_wall, f0_dev, f0_wall, f4_dev, f4_wall, fe_wall)):
                        rows[k].append(v)
            say(case=name, gsd=gsd, raster=[frame.width, frame.height], contributors=contributors, occupied=occupied, filled_r4=filled,
                atomics=st["atomics"], atomics_per_contributor=round(st["atomics"] / max(contributors, 1), 4),
                map_bytes=frame.width * frame.height * 17, ms={k: spread(v) for k, v in rows.items()})

    if args.stand_in:
        with capi.Context(0) as ctx:
            ctx.timing_enable(True)
            ctx.upload_cloud(x, y, z)
            lo = np.quantile(x, 0.38), np.quantile(y, 0.38)
            hi = np.quantile(x, 0.62), np.quantile(y, 0.62)
            box = (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1])
            colours = (synth._hash32(np.arange(args.points, dtype=np.uint32)) & np.uint32(0xFFFFFF))
            for name, has in (("box", box), ("every row", np.ones(args.points, bool))):
                words = torch.from_numpy((colours | (has.astype(np.uint32) << 24)).view(np.int32)).to("cuda:0")
                torch.cuda.synchronize()
                print(f"{name}: {int(has.sum())} rows with the has bit", file=sys.stderr, flush=True)
                measure(ctx, "stand-in, " + name, has.astype(np.uint8), lambda: ctx.ortho_add_packed(int(words.data_ptr())))
        return

    cd = synth.camera_dict("cfg")
    W, H = cd["image_width"], cd["image_height"]
    poses, _ = synth.make_trajectory(args.frames, seed=synth.SEED)
    smooth, colour = pipeline.HipEngine(0), pipeline.HipEngine(0)
    colour.configure(cd)
    e = x[:0]
    colour.ctx.upload_cloud(e, e, e)  # (the image uploads ask for a cloud)
    colour.set_keyframes(poses)
    for f in range(args.frames):
        colour.ctx.upload_image(f, synth.make_image(f, W, H))
    colour.ctx.synchronize()
    if not args.streamed:
        ctx = colour.ctx
        ctx.timing_enable(True)
        ctx.upload_cloud(x, y, z)
        ctx.colorize(download=False)
        has = (ctx.download_result_packed() >> 24).astype(np.uint8)
        measure(ctx, "C3 one-shot", has, lambda: ctx.ortho_add(0))
        return
    p = capi.default_mls_params()  # VOXEL_GRID_DILATION 1 mm x 4: the reference's configuration
    cs = pipeline.CloudSmooth(smooth, p)
    on = dict(frame="auto", gsd=0.005, fill_radius=4, xyz=xyz, viewer=np.asarray(poses, np.float64).reshape(-1, 7)[:, :3].mean(axis=0))
    for ortho in (None, on, None, on):
        smooth.upload_cloud(x, y, z)
        t0 = time.perf_counter()
        coloured = sum(c["count"] for c in cs.process_and_colourise_streamed(colour, 1 << args.chunk_log2, download=False, ortho=ortho))
        st = {k: v for k, v in cs.streamed_colour.items() if not isinstance(v, list)}
        out = cs.ortho_output
        say(case="streamed chain", ortho=ortho is not None, coloured=coloured, seconds=round(time.perf_counter() - t0, 3), stats=st,
            bytes_leaving=0 if out is None else sum(v.nbytes for v in out.values() if hasattr(v, "nbytes")))


if __name__ == "__main__":
    main()
