#!/usr/bin/env python3
"""The planar facets ("Planar facets") at scale, on one MI355X.  Run it under one `timeout`.

    python scripts/facets_probe.py [--points N] [--frames F] [--radii 0.03,0.1] [--repeats 3] [--no-ortho]

The 10 M-point scene: per link radius, pcp_estimate_normals at that radius (the one existing pass that walks the same
neighbours) and pcp_facets at it, in one session: the kernels' device time (PCP_K_MISC) and the host's wall clock, median
[min .. max] of --repeats rounds after one warm-up round; facet points, components, facets, the largest facet and the planar
count.  Then, unless --no-ortho: the colour result under --frames keyframes, one whole-map pcp_ortho_add at --gsd against the
pcp_ortho_add_facet of every planar facet on its own fitted frame (add, finish, fetch per facet).
The split of pcp_facets over its kernels (records, union, flatten, stats, moments) is what
    rocprofv3 --kernel-trace --stats -- python scripts/facets_probe.py --no-ortho --repeats 1
prints per k_fa_* / k_cc_flatten row; this script reports the call as a whole.
PCP_HIP_LIBRARY selects another build of the same ABI.  One JSON line per measurement on stdout.  Not collected by pytest."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--radii", default="0.03,0.1")
    ap.add_argument("--gsd", type=float, default=0.005)
    ap.add_argument("--min-points", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-ortho", action="store_true")
    args = ap.parse_args()
    import numpy as np

    from pointcloudprocessor_amd import capi, pipeline, synth

    def say(**kw):
        print(json.dumps(kw), flush=True)

    say(library=os.environ.get("PCP_HIP_LIBRARY", "default"), points=args.points)
    x, y, z, _ = synth.make_cloud(args.points, seed=synth.SEED)
    xyz = np.stack([x, y, z], axis=1)
    eng = pipeline.HipEngine(0)
    ctx = eng.ctx
    ctx.timing_enable(True)

    def timed(fn):
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return ctx.timing_get(capi.K_MISC)[0], (time.perf_counter() - t0) * 1e3, out

    ctx.upload_cloud(x, y, z)
    fac = None
    for radius in [float(r) for r in args.radii.split(",")]:
        rows = {k: [] for k in ("normals_dev", "normals_wall", "facets_dev", "facets_wall")}
        for rep in range(1 + args.repeats):
            n_dev, n_wall, valid = timed(lambda: ctx.estimate_normals(radius))
            f_dev, f_wall, fac = timed(lambda: ctx.facets(link_radius=radius, min_points=args.min_points))
            if rep >= 1:
                for k, v in zip(rows, (n_dev, n_wall, f_dev, f_wall)):
                    rows[k].append(v)
        planes = np.array([capi.facet_plane_host(xyz[i], r) for i, r in zip(fac["ids"], fac["rows"])]).reshape(-1, 7)
        say(case="facets", radius=radius, valid_normals=valid, facet_points=fac["facet_points"], components=fac["components"],
            facets=fac["facets"], largest=int(fac["rows"][:, 0].max()) if fac["facets"] else 0,
            planar=int((planes[:, 6] <= 0.01).sum()), ms={k: spread(v) for k, v in rows.items()})
    if args.no_ortho:
        return
    cd = synth.camera_dict("cfg")
    W, H = cd["image_width"], cd["image_height"]
    poses, _ = synth.make_trajectory(args.frames, seed=synth.SEED)
    eng.configure(cd)
    eng.set_keyframes(poses)
    for f in range(args.frames):
        ctx.upload_image(f, synth.make_image(f, W, H))
    ctx.upload_cloud(x, y, z)
    ctx.colorize(download=False)
    has = (ctx.download_result_packed() >> 24).astype(np.uint8)
    col = pipeline.PointCloudColorizer(eng)
    radius = float(args.radii.split(",")[-1])
    fac = col.facets(xyz=xyz, normal_radius=radius, link_radius=radius, min_points=args.min_points)
    frame = capi.ortho_fit_frame_host(xyz, args.gsd, has=has, viewer=eng.mean_keyframe_position)
    whole = {k: [] for k in ("add_dev", "add_wall")}
    for rep in range(1 + args.repeats):
        ctx.ortho_begin(frame)
        dev, wall, contributors = timed(lambda: ctx.ortho_add(0))
        ctx.ortho_end()
        if rep >= 1:
            whole["add_dev"].append(dev)
            whole["add_wall"].append(wall)
    say(case="whole-map ortho_add", gsd=args.gsd, raster=[frame.width, frame.height], contributors=contributors,
        ms={k: spread(v) for k, v in whole.items()})
    t0 = time.perf_counter()
    dev, wall, maps = timed(lambda: col.ortho_maps_by_facet(args.gsd, xyz=xyz, facets=fac))
    say(case="ortho maps by facet", gsd=args.gsd, planar_facets=len(maps), contributors=sum(m["contributors"] for m in maps),
        pixels=sum(m["frame"]["width"] * m["frame"]["height"] for m in maps), device_ms=round(dev, 3), wall_ms=round(wall, 3),
        seconds=round(time.perf_counter() - t0, 3))


if __name__ == "__main__":
    main()
