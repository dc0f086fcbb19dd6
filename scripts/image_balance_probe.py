#!/usr/bin/env python3
"""The keyframe colour balance ("Image balance") at scale, on one MI355X; fills profiles/image_balance_probe.md.
Run it under one `timeout`; every child step has a time limit of its own and a failed step ends the run.

    python scripts/image_balance_probe.py [--out profiles/image_balance_probe.md] [--frames 256] [--repeats 20]
    python scripts/image_balance_probe.py --case 1920x1080,noise        # one case only (what the parent runs under rocprofv3)

Kernel times: Context.image_balance (the kernels the upload path runs) at 1920x1080 and 4096x3000 on noise, a constant image
and a ramp + blob image, the defaults.  The library times all of them in one slot (PCP_K_MISC, hipEvents): that total is
reported, and the split by kernel comes from `rocprofv3 --kernel-trace --stats` over a child run of the same case.
End to end: --frames keyframes at 1080p through upload_image_async with balance off and on (wall clock to the synchronise),
and image_balance_host on one thread for one keyframe, the host-side cost it replaces.  Not collected by pytest."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(1920, 1080), (4096, 3000)]
KINDS = ["noise", "constant", "looks_real"]
KERNELS = ["k_pack_bgr16", "k_balance_hist", "k_balance_lut", "k_balance_apply", "k_balance_unpack"]


def picture(kind, w, h):
    import _image_balance_ref as ref

    return ref.looks_real(w, h) if kind == "looks_real" else ref.image(kind, w, h)


def run_case(w, h, kind, repeats):
    """the device form `repeats` times after two warm-ups: K_MISC device ms per call (median, min, max)"""
    from pointcloudprocessor_amd import capi

    im = picture(kind, w, h)
    ms = []
    with capi.Context(0) as ctx:
        ctx.timing_enable(True)
        for rep in range(2 + repeats):
            ctx.timing_reset()
            ctx.image_balance(im, True)
            if rep >= 2:
                ms.append(ctx.timing_get(capi.K_MISC)[0])
    return dict(size=f"{w}x{h}", image=kind, calls=repeats, k_misc_ms=dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4),
                                                                               max=round(max(ms), 4)))


def kernel_split(w, h, kind, repeats):
    """average us per launch of each kernel, from rocprofv3's kernel statistics of a child run of the case"""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--",
               sys.executable, os.path.abspath(__file__), "--case", f"{w}x{h},{kind}", "--repeats", str(repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise SystemExit(f"rocprofv3 child failed ({p.returncode}): {p.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                for k in KERNELS:
                    if k + "(" in name or k + "<" in name or name.endswith(k):
                        out[k] = dict(launches=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2),
                                      min_us=round(float(row["MinNs"]) / 1e3, 2), max_us=round(float(row["MaxNs"]) / 1e3, 2))
        return out


def upload_loop(frames, balance):
    import numpy as np
    import torch

    from pointcloudprocessor_amd import capi, synth

    w, h = 1920, 1080
    ring = torch.empty((8, h, w, 3), dtype=torch.uint8).pin_memory()
    rn = ring.numpy()
    for k in range(8):
        rn[k] = synth.make_image(k, w, h)
    cd = synth.camera_dict("tiny")
    cd.update(image_width=w, image_height=h)
    with capi.Context(0) as ctx:
        ctx.set_camera(capi.camera_from_dict(cd))
        e = np.zeros(0, np.float32)
        ctx.upload_cloud(e, e, e)
        poses, _ = synth.make_trajectory(frames)
        ctx.set_frames(poses)
        ctx.set_image_balance(True if balance else None)
        walls = []
        for rep in range(4):
            ctx.synchronize()
            t0 = time.perf_counter()
            for f in range(frames):
                ctx.upload_image_async(f, rn[f % 8])
            ctx.synchronize()
            if rep >= 1:
                walls.append((time.perf_counter() - t0) * 1e3)
    return dict(frames=frames, balance=balance, wall_ms=dict(median=round(statistics.median(walls), 2), min=round(min(walls), 2),
                                                             max=round(max(walls), 2)))


def host_cost():
    from pointcloudprocessor_amd import capi, synth

    im = synth.make_image(0, 1920, 1080)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        capi.image_balance_host(im, True)
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(image_balance_host_1080p_ms=round(min(t), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_balance_probe.md"))
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--case")
    args = ap.parse_args()
    if args.case:
        size, kind = args.case.split(",")
        w, h = (int(v) for v in size.split("x"))
        print(json.dumps(run_case(w, h, kind, args.repeats)), flush=True)
        return
    rows = []
    for w, h in SIZES:
        for kind in KINDS:
            r = run_case(w, h, kind, args.repeats)
            r["kernels"] = kernel_split(w, h, kind, args.repeats)
            print(json.dumps(r), flush=True)
            rows.append(r)
    loops = [upload_loop(args.frames, False), upload_loop(args.frames, True)]
    host = host_cost()
    print(json.dumps(dict(loops=loops, host=host)), flush=True)
    with open(args.out, "w") as f:
        f.write("# Image balance probe\n\nOne MI355X, `python scripts/image_balance_probe.py`.  `pcp_image_balance` with the defaults (8 x 8 tiles, clip 1.0, "
                "gamma 0.8, both stages).\nK_MISC: the hipEvent time of all kernels of one call (pack, hist, lut, apply, unpack), median [min .. max] ms over "
                f"{args.repeats} calls.\nPer kernel: average us per launch [min .. max] from `rocprofv3 --kernel-trace --stats` over a child run of the same "
                "case (one timing slot holds them all, so hipEvents do not split them).\n\n")
        f.write("| size | image | K_MISC ms | " + " | ".join(k + " us" for k in KERNELS) + " |\n|---|---|---|" + "---|" * len(KERNELS) + "\n")
        for r in rows:
            m = r["k_misc_ms"]
            cells = []
            for k in KERNELS:
                s = r["kernels"].get(k)
                cells.append(f"{s['avg_us']} [{s['min_us']} .. {s['max_us']}]" if s else "not measured")
            f.write(f"| {r['size']} | {r['image']} | {m['median']} [{m['min']} .. {m['max']}] | " + " | ".join(cells) + " |\n")
        f.write(f"\n## End to end\n\n{args.frames} keyframes at 1920x1080 through `upload_image_async` from pinned memory, wall clock to the synchronise, "
                "median [min .. max] ms over 3 rounds after one warm-up:\n\n| balance | wall ms |\n|---|---|\n")
        for lp in loops:
            m = lp["wall_ms"]
            f.write(f"| {'on' if lp['balance'] else 'off'} | {m['median']} [{m['min']} .. {m['max']}] |\n")
        f.write(f"\n`image_balance_host` on one thread of the same box, one 1920x1080 keyframe: {host['image_balance_host_1080p_ms']} ms (best of 3).\n")


if __name__ == "__main__":
    main()
