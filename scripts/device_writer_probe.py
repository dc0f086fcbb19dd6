#!/usr/bin/env python3
"""What the device PCD writer (--deviceWriter 1, DESIGN.md "Device PCD writer") costs and saves.

    python scripts/device_writer_probe.py [--points N] [--frames F] [--runs 3] [--parent-exe PATH] [--streamed]

cli      the command line on an N-point map (default 10 M) with F keyframes at 1920x1080, --skip_filtered_dumps 1: the phases
         of its timing file (PCP_CLI_TIMING) for the host writer and for --deviceWriter 1, `runs` runs each, alternating.  The
         host-writer runs use --parent-exe when given (a build of the parent commit), else this tree with --deviceWriter 0.
library  pcp_colour_compact_ascii over the whole coloured map in one call: wall time of the call, the PCP_K_MISC kernel
         time inside it (pcp_timing_get: has flags, compaction, lengths, scan, text) and the bytes of text.
streamed --streamed: the command line with --enableMLS 1 --streamColour 1 on a smaller map (the whole C3 chain at the
         reference's configuration writes ~300 GB of text; say what ran), with and without --deviceWriter 1.

One JSON line per measurement on stdout.  Not collected by pytest."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dataset(d, n, F, W, H, masks):
    import numpy as np

    from pointcloudprocessor_amd import synth

    x, y, z, inten = synth.make_cloud(n)
    hdr = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
           f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(os.path.join(d, "scans.pcd"), "wb") as fh:
        fh.write(hdr.encode())
        fh.write(np.stack([x, y, z, inten], 1).astype(np.float32).tobytes())
    poses, ts = synth.make_trajectory(F)
    with open(os.path.join(d, "odo.txt"), "w") as fh:
        for k, (t, p) in enumerate(zip(ts, poses)):
            fh.write(synth.odometry_line(t, p))
            with open(os.path.join(d, "%f.ppm" % t), "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (W, H) + synth.make_image(k, W, H)[:, :, ::-1].tobytes())
            if masks:
                with open(os.path.join(d, "%f.pgm" % t), "wb") as g:
                    g.write(b"P5\n%d %d\n255\n" % (W, H) + synth.make_mask(k, W, H).tobytes())


def cli(exe, d, tag, extra, masks=False):
    out = os.path.join(d, tag) + "/"
    os.makedirs(out)
    env = dict(os.environ, PCP_CLI_TIMING=out + "t.json")
    cmd = [exe, "-p", d + "/scans.pcd", "-o", d + "/odo.txt", "-i", d + "/", "-t", out] + (["-m", d + "/"] if masks else []) + extra
    t0 = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=out)
    wall = time.perf_counter() - t0
    ph = json.load(open(out + "t.json")) if p.returncode == 0 else {"error": p.stderr[-300:]}
    sizes = {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out)) if f.endswith(".pcd")}
    shutil.rmtree(out, ignore_errors=True)
    return dict(wall_s=round(wall, 3), files=sizes, **{a: round(b, 4) for a, b in ph.items() if isinstance(b, float)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-exe", default=None, help="PointCloudProcessor built from the parent commit")
    ap.add_argument("--streamed", action="store_true")
    ap.add_argument("--streamed-points", type=int, default=100_000)
    args = ap.parse_args()
    from pointcloudprocessor_amd import capi, host_build, synth

    exe = host_build.build()["PointCloudProcessor"]
    W, H = 1920, 1080
    d = tempfile.mkdtemp(prefix="pcp_writer_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        dataset(d, args.points, args.frames, W, H, masks=False)
        host_exe, host_flags = (args.parent_exe, []) if args.parent_exe else (exe, ["--deviceWriter", "0"])
        for r in range(args.runs):
            for name, e, flags in (("host_writer", host_exe, host_flags), ("device_writer", exe, ["--deviceWriter", "1"])):
                res = cli(e, d, f"{name}{r}", ["--skip_filtered_dumps", "1"] + flags)
                print(json.dumps(dict(part="cli", writer=name, parent_build=bool(args.parent_exe) and name == "host_writer", run=r,
                                      points=args.points, frames=args.frames, **res)), flush=True)
        # the library call alone
        import numpy as np

        cd = synth.camera_dict("cfg")
        x, y, z, _ = synth.make_cloud(args.points)
        poses, _ = synth.make_trajectory(args.frames)
        ctx = capi.Context(0)
        ctx.set_camera(capi.camera_from_dict(cd))
        ctx.upload_cloud(x, y, z)
        ctx.set_frames(poses)
        for f in range(args.frames):
            ctx.upload_image(f, synth.make_image(f, W, H))
        ctx.colorize(download=False)
        out = np.empty(args.points * capi.ascii_row_bound(capi.ROWS_XYZRGB), np.uint8)
        out[:] = 0  # touched before the timed calls
        for r in range(args.runs):
            ctx.timing_enable(True)
            ctx.timing_reset()
            nbytes, rows = capi.C.c_int64(), capi.C.c_int64()
            t0 = time.perf_counter()
            ctx._check(ctx.lib.pcp_colour_compact_ascii(ctx.h, 0, capi.C.c_int64(0), capi.C.c_int64(args.points), capi.C.c_int64(out.size),
                                                        capi._ptr(out), capi.C.byref(rows), capi.C.byref(nbytes)))
            wall = time.perf_counter() - t0
            ms, launches = ctx.timing_get(6)  # PCP_K_MISC
            ctx.timing_enable(False)
            t0 = time.perf_counter()
            binary = ctx.colour_compact()
            wall_bin = time.perf_counter() - t0
            print(json.dumps(dict(part="library", run=r, rows=rows.value, text_bytes=nbytes.value, call_wall_s=round(wall, 4),
                                  misc_kernels_ms=round(ms, 3), misc_launches=launches,
                                  text_GBps_of_kernels=round(nbytes.value / (ms * 1e-3) / 1e9, 2) if ms > 0 else None,
                                  download_and_host_s=round(wall - ms * 1e-3, 4), binary_compact_wall_s=round(wall_bin, 4),
                                  binary_rows=int(binary["count"]))), flush=True)
        ctx.close()
        if args.streamed:
            sd = os.path.join(d, "streamed")
            os.makedirs(sd)
            dataset(sd, args.streamed_points, 8, W, H, masks=True)
            common = ["--enableMLS", "1", "--streamColour", "1", "--fuseMasks", "1", "--skip_filtered_dumps", "1"]
            for r in range(2):
                for name, flags in (("host_writer", ["--deviceWriter", "0"]), ("device_writer", ["--deviceWriter", "1"])):
                    res = cli(exe, sd, f"s_{name}{r}", common + flags, masks=True)
                    print(json.dumps(dict(part="streamed", writer=name, run=r, points=args.streamed_points, frames=8, **res)), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
