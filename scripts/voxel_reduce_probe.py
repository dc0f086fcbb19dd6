#!/usr/bin/env python3
"""The voxel-grid output ("Voxel-grid output") at scale, on one MI355X.  Run it under one `timeout`.

    python scripts/voxel_reduce_probe.py [--points N] [--frames F] [--chunk-log2 28] [--leaf 0.005] [--skip-streamed] [--skip-one-shot]

C3 streamed: the streamed chain at the reference's configuration (VOXEL_GRID_DILATION 1 mm x 4, 256 keyframes at 1920x1080, as
scripts/stream_colour_probe.py sets it up), twice in one session: sweep B with the full download of the coloured rows, then
sweep B with output_leaf and download=False, where only the reduced rows leave the device.
C3 one-shot: the one-shot colour result of the map, add + finish + fetch at 5 mm and 50 mm.
One JSON line per measurement on stdout, progress on stderr.  Not collected by pytest."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--chunk-log2", type=int, default=28)
    ap.add_argument("--leaf", type=float, default=0.005)
    ap.add_argument("--skip-streamed", action="store_true")
    ap.add_argument("--skip-one-shot", action="store_true")
    args = ap.parse_args()
    import torch

    from pointcloudprocessor_amd import capi, pipeline, synth

    def used():
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    def say(**kw):
        print(json.dumps(kw), flush=True)

    cd = synth.camera_dict("cfg")
    W, H = cd["image_width"], cd["image_height"]
    x, y, z, _ = synth.make_cloud(args.points, seed=synth.SEED)
    poses, _ = synth.make_trajectory(args.frames, seed=synth.SEED)
    smooth, colour = pipeline.HipEngine(0), pipeline.HipEngine(0)
    base = used()
    colour.configure(cd)
    e = x[:0]
    colour.upload_cloud(e, e, e)  # (the image uploads ask for a cloud)
    colour.ctx.set_frames(poses)
    for f in range(args.frames):
        colour.ctx.upload_image(f, synth.make_image(f, W, H))
    colour.ctx.synchronize()
    images = used() - base
    print(f"images resident: {images / 1e9:.2f} GB", file=sys.stderr, flush=True)

    if not args.skip_one_shot:
        ctx = colour.ctx
        ctx.upload_cloud(x, y, z)
        ctx.colorize(download=False)
        ctx.synchronize()
        coloured = ctx.colour_compact(capacity=0)["count"]
        for leaf in (0.005, 0.05):
            for rep in range(2):  # (the second repetition is the one to quote: the first pays the allocations)
                t0 = time.perf_counter()
                ctx.voxel_reduce_begin(leaf)
                ctx.voxel_reduce_add()
                t1 = time.perf_counter()
                ctx.voxel_reduce_finish()
                t2 = time.perf_counter()
                out = ctx.voxel_reduce_fetch()
                t3 = time.perf_counter()
                st = ctx.voxel_reduce_stats()
                ctx.voxel_reduce_end()
                say(case="one_shot", points=args.points, coloured=coloured, leaf=leaf, repetition=rep,
                    add_s=round(t1 - t0, 5), finish_s=round(t2 - t1, 5), fetch_s=round(t3 - t2, 5), total_s=round(t3 - t0, 5),
                    table_bytes=52 * st["slots"], fetched_bytes=int(sum(v.nbytes for v in out.values())), **st)
        ctx.upload_cloud(e, e, e)

    if not args.skip_streamed:
        smooth.upload_cloud(x, y, z)
        cs = pipeline.CloudSmooth(smooth, capi.default_mls_params())
        for variant, kw in (("full_download", dict(download=True)), ("voxel_output", dict(download=False, output_leaf=args.leaf))):
            t0 = time.perf_counter()
            peak = used()
            chunks = rows = 0
            for part in cs.process_and_colourise_streamed(colour, 1 << args.chunk_log2, **kw):
                chunks += 1
                rows += part["count"] if "count" in part else len(part["index"])
                peak = max(peak, used())
                print(f"{variant}: chunk {chunks}, {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            total = time.perf_counter() - t0
            peak = max(peak, used())
            st, sm = dict(cs.streamed_colour), cs.streamed
            begin = sum(sm["begin_seconds"][k] for k in ("filter_fit_voxels", "sweep0", "sweep1_threshold"))
            vox = st.pop("voxel", None)
            extra = {}
            if vox is not None:
                out = cs.voxel_output
                per_wave = max(1, (vox["rows"] + 63) // 64)
                extra = dict(leaf=args.leaf, voxels=vox["voxels"], table_slots=vox["slots"], table_bytes=52 * vox["slots"],
                             growths=vox["growths"], partials_per_wavefront=round(vox["wave_partials"] / per_wave, 3),
                             adds_per_wavefront=round(vox["global_adds"] / per_wave, 3), rows_added=vox["rows"],
                             fetched_bytes=int(sum(v.nbytes for v in out.values())))
                for k in ("voxel_add_s", "voxel_finish_s"):
                    st[k] = round(st[k], 4)
                st["voxel_add_chunk_s"] = [round(v, 4) for v in st["voxel_add_chunk_s"]]
            say(case="streamed", variant=variant, points=args.points, frames=args.frames, chunk_capacity=1 << args.chunk_log2,
                yielded_rows=rows, begin_s=round(begin, 3), total_s=round(total, 3), peak_device_bytes=int(peak - base),
                image_bytes=int(images), **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}, **extra)
    smooth.close()
    colour.close()


if __name__ == "__main__":
    main()
