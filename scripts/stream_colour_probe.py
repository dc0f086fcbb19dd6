#!/usr/bin/env python3
"""Streamed colourisation of the whole C3 map at the reference's own MLS configuration (VOXEL_GRID_DILATION 1 mm x 4,
PointCloudProcessor.cpp:67-86) against 256 keyframes at 1920x1080: the smoothing chain's chunks are handed to a second
context on the device, sweep A merges their depth maps, sweep B colours them against the merged maps and compacts the
coloured rows, which are downloaded chunk by chunk and dropped (pipeline.CloudSmooth.process_and_colourise_streamed).

    python scripts/stream_colour_probe.py [--points N] [--frames F] [--chunk-log2 28] [--labels] [--count-only]

One JSON line on stdout: seconds of the stream's begin, of sweep A and sweep B and their sum, rows and coloured rows, and the
device memory in use (hipMemGetInfo; both contexts together -- the buffers only grow, so the value after the last chunk is
the peak), with the share the images hold.  --count-only leaves the coloured rows on the device (only their count comes back):
what the device work costs without the download.  Progress goes to stderr.  Not collected by pytest."""
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
    ap.add_argument("--labels", action="store_true", help="fuse segmentation labels too (masks uploaded)")
    ap.add_argument("--count-only", action="store_true", help="leave the coloured rows on the device")
    args = ap.parse_args()
    import torch

    from pointcloudprocessor_amd import capi, pipeline, synth

    def used():
        free, total = torch.cuda.mem_get_info(0)
        return total - free

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
        if args.labels:
            colour.ctx.upload_mask(f, synth.make_mask(f, W, H))
    colour.ctx.synchronize()
    images = used() - base
    print(f"images resident: {images / 1e9:.2f} GB", file=sys.stderr, flush=True)
    smooth.upload_cloud(x, y, z)
    cs = pipeline.CloudSmooth(smooth, capi.default_mls_params())
    t0 = time.perf_counter()
    peak = used()
    chunks = rows = 0
    checksum = 0
    for part in cs.process_and_colourise_streamed(colour, 1 << args.chunk_log2, fuse_labels=args.labels,
                                                  download=not args.count_only):
        chunks += 1
        got = part["count"] if args.count_only else len(part["index"])
        rows += got
        if not args.count_only:
            checksum ^= int(part["rgb"][::4097].astype("u8").sum())  # the rows reached the host
        peak = max(peak, used())
        print(f"chunk {chunks}: {got} coloured rows, {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    total = time.perf_counter() - t0
    st, sm = cs.streamed_colour, cs.streamed
    begin = sum(sm["begin_seconds"][k] for k in ("filter_fit_voxels", "sweep0", "sweep1_threshold"))
    print(json.dumps(dict(points=args.points, frames=args.frames, camera="cfg 1920x1080", chunk_capacity=1 << args.chunk_log2,
                          labels=bool(args.labels), downloaded=not args.count_only, chunks=st["chunks"], rows_before_last_filter=sm["rows"], rows=st["rows"],
                          coloured=st["coloured"], chunks_with_colour=chunks, begin_s=round(begin, 3),
                          sweep_a_s=round(st["sweep_a_s"], 3), sweep_b_s=round(st["sweep_b_s"], 3), total_s=round(total, 3),
                          peak_device_bytes=int(peak - base), image_bytes=int(images), rgb_checksum=checksum)), flush=True)
    smooth.close()
    colour.close()


if __name__ == "__main__":
    main()
