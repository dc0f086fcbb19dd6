#!/usr/bin/env python3
"""The unrolled maps of cylindrical facets ("Cylindrical facets") at scale, on one MI355X.  Run it under one `timeout`.

    python scripts/cylinder_probe.py [--points N] [--repeats 5]

The 10 M-point map with every has bit set, the words in device memory (ortho_add_packed), at gsd 5 mm and 50 mm: a planar frame
fitted to the map, and beside it a cylinder's frame of the same raster -- a vertical axis through the map's centroid, R chosen
so that the circumference is the planar raster's width, the same height -- add (scatter + payload), finish without a fill and
with R = 4, atomics per contributor from the stats.  Two warm-up rounds, then --repeats rounds; the kernels' device time
(PCP_K_MISC) and the host's wall clock, median [min .. max].  One JSON line per measurement on stdout.  Not collected by pytest."""
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
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch

    from pointcloudprocessor_amd import capi, synth

    def say(**kw):
        print(json.dumps(kw), flush=True)

    x, y, z, _ = synth.make_cloud(args.points, seed=synth.SEED)
    xyz = np.stack([x, y, z], axis=1)
    centre = xyz.mean(axis=0, dtype=np.float64)
    top = float(z.max())

    def timed(ctx, fn):
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return ctx.timing_get(capi.K_MISC)[0], (time.perf_counter() - t0) * 1e3, out

    with capi.Context(0) as ctx:
        ctx.timing_enable(True)
        ctx.upload_cloud(x, y, z)
        colours = synth._hash32(np.arange(args.points, dtype=np.uint32)) & np.uint32(0xFFFFFF)
        words = torch.from_numpy((colours | np.uint32(1 << 24)).view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        for gsd in (0.005, 0.05):
            plane = capi.ortho_fit_frame_host(xyz, gsd)
            g = float(np.float32(gsd))
            radius = plane.width * g / (2 * np.pi)
            cyl = capi.cyl_frame(dict(c=(centre[0], centre[1], top + g), a=(0, 0, -1), e=(1, 0, 0), b=(0, -1, 0), radius=radius, gsd=gsd,
                                      width=plane.width, height=plane.height, d_min=-radius, d_max=1000.0, side=1))
            for name, begin, frame in (("planar", ctx.ortho_begin, plane), ("cylinder", ctx.ortho_begin_cyl, cyl)):
                rows = {k: [] for k in ("add_dev", "add_wall", "finish0_dev", "finish4_dev")}
                for rep in range(2 + args.repeats):
                    begin(frame)
                    a_dev, a_wall, contributors = timed(ctx, lambda: ctx.ortho_add_packed(int(words.data_ptr())))
                    f0_dev, _, (occupied, _) = timed(ctx, lambda: ctx.ortho_finish(0))
                    f4_dev, _, (_, filled) = timed(ctx, lambda: ctx.ortho_finish(4))
                    st = ctx.ortho_stats()
                    ctx.ortho_end()
                    if rep >= 2:
                        for k, v in zip(rows, (a_dev, a_wall, f0_dev, f4_dev)):
                            rows[k].append(v)
                say(case=name, gsd=gsd, raster=[frame.width, frame.height], contributors=contributors, occupied=occupied, filled_r4=filled,
                    atomics=st["atomics"], atomics_per_contributor=round(st["atomics"] / max(contributors, 1), 4),
                    ms={k: spread(v) for k, v in rows.items()})


if __name__ == "__main__":
    main()
