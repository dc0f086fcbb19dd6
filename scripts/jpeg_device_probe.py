"""Device JPEG reconstruction (pcp_upload_image_jpeg) on the MI355X: what it costs and what it saves.

  python3 scripts/jpeg_device_probe.py --out profiles/jpeg_device_probe.json [--parent TREE] [--cli-frames 256]

  * host: wall seconds of one `image_dump` process per keyframe file on a tmpfs (best of --reps), full decode to BGR vs
    entropy decode to the coefficient blob; with --parent TREE (a built checkout of the parent commit) also the parent's full
    decode.  The process figures include start-up, the file read and the output write (a few ms);
  * bytes: blob vs BGR;
  * device: wall time of one synchronised upload per keyframe (pcp_upload_image_jpeg vs pcp_upload_image from host BGR),
    median of --reps, every reconstructed keyframe checked against the host decoder byte for byte;
  * --kernels-only: only the uploads (run it under rocprofv3 --kernel-trace --stats for k_jpeg_idct / k_jpeg_pixels);
  * --cli-frames N: the command line on N 4096x3000 JPEG keyframes (8 distinct pictures) on a tmpfs, 16 decoder threads,
    this tree and --parent alternating twice: images_decode_and_upload_wall_s, images_decode_thread_seconds, and the colour
    file of both compared byte for byte.
Pictures: synth.make_image frames (noisy) and a smooth gradient picture, Pillow quality 92, 4:2:0."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def smooth_picture(k, w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    im = np.stack([128 + 100 * np.sin(x / 400.0 + y / 700.0 + k), 128 + 90 * np.cos(x / 300.0 - y / 500.0),
                   128 + 80 * np.sin((x + y) / 900.0)], 2)
    return np.clip(im, 0, 255).astype(np.uint8)


def timed(cmd, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True, capture_output=True)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def read_bgr(path):
    raw = open(path, "rb").read()
    head, _, body = raw.partition(b"\n")
    w, h, c = map(int, head.split())
    return np.frombuffer(body, np.uint8).reshape(h, w, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parent", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--cli-frames", type=int, default=0)
    ap.add_argument("--cli-reps", type=int, default=2, help="alternating runs of each tree")
    ap.add_argument("--cli-only", action="store_true", help="only the command-line leg")
    a = ap.parse_args()

    from PIL import Image

    from pointcloudprocessor_amd import _build, capi, host_build, synth

    _build.build()
    bins = host_build.build()
    dump = bins["image_dump"]
    if a.parent:
        a.parent = os.path.abspath(a.parent)
    pdump = os.path.join(a.parent, "pointcloudprocessor_amd/host/bin/image_dump") if a.parent else None
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    d = tempfile.mkdtemp(prefix="pcp_jpeg_probe_", dir=base)
    res = {"filesystem": base, "reps": a.reps, "cases": []}
    try:
        for (w, h) in ([] if a.cli_only else [(4096, 3000), (1920, 1080)]):
            for kind in ("synth", "smooth"):
                pic = synth.make_image(0, w, h)[:, :, ::-1] if kind == "synth" else smooth_picture(0, w, h)
                jp = os.path.join(d, f"{kind}_{w}x{h}.jpg")
                Image.fromarray(np.ascontiguousarray(pic)).save(jp, quality=92)
                subprocess.run([dump, jp, jp + ".raw"], check=True)
                subprocess.run([dump, jp, jp + ".blob", "coeffs"], check=True)
                bgr = np.ascontiguousarray(read_bgr(jp + ".raw"))
                blob = np.fromfile(jp + ".blob", np.uint8)
                case = {"image": f"{w}x{h}", "picture": kind, "jpeg_bytes": os.path.getsize(jp), "blob_bytes": int(blob.size),
                        "bgr_bytes": int(bgr.size)}
                if not a.kernels_only:
                    case["host_full_decode_s"] = round(timed([dump, jp, jp + ".raw"], a.reps), 4)
                    case["host_entropy_only_s"] = round(timed([dump, jp, jp + ".blob", "coeffs"], a.reps), 4)
                    if pdump:
                        case["parent_host_full_decode_s"] = round(timed([pdump, jp, jp + ".praw"], a.reps), 4)
                        assert np.array_equal(read_bgr(jp + ".praw"), bgr), "parent and branch decoders disagree"
                        case["host_speedup_vs_parent"] = round(case["parent_host_full_decode_s"] / case["host_entropy_only_s"], 2)
                cd = synth.camera_dict("tiny")
                cd.update(image_width=w, image_height=h)
                with capi.Context(0) as ctx:
                    ctx.set_camera(capi.camera_from_dict(cd))
                    x, y, z, _ = synth.make_cloud(1000)
                    ctx.upload_cloud(x, y, z)
                    ctx.set_frames(synth.make_trajectory(2)[0])
                    ctx.set_image_adjust(True)
                    tj, tb = [], []
                    for _ in range(a.reps + 1):
                        t0 = time.perf_counter()
                        ctx.upload_image_jpeg(0, blob)
                        ctx.synchronize()
                        tj.append(time.perf_counter() - t0)
                        t0 = time.perf_counter()
                        ctx.upload_image(1, bgr)
                        ctx.synchronize()
                        tb.append(time.perf_counter() - t0)
                    g0, _ = ctx.download_image(0)
                    g1, _ = ctx.download_image(1)
                    assert np.array_equal(g0, g1), f"device reconstruction differs from the host decoder ({kind} {w}x{h})"
                case["upload_jpeg_sync_s"] = round(statistics.median(tj[1:]), 5)
                case["upload_bgr_sync_s"] = round(statistics.median(tb[1:]), 5)
                case["device_equals_host"] = True
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
        if a.cli_frames and not a.kernels_only:
            res["cli"] = cli_leg(a, bins["PointCloudProcessor"], d, synth, Image)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res.get("cli", {})))


def cli_leg(a, exe, d, synth, Image):
    W, H, N = 4096, 3000, a.cli_frames
    n_points = 1_000_000
    x, y, z, inten = synth.make_cloud(n_points)
    pcd = os.path.join(d, "scans.pcd")
    hdr = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\n"
           f"TYPE F F F F\nCOUNT 1 1 1 1\nWIDTH {n_points}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n_points}\nDATA binary\n")
    with open(pcd, "wb") as fh:
        fh.write(hdr.encode())
        fh.write(np.stack([x, y, z, inten], 1).astype(np.float32).tobytes())
    poses, ts = synth.make_trajectory(N)
    imgs = os.path.join(d, "img")
    os.makedirs(imgs)
    distinct = []
    for k in range(8):
        fn = os.path.join(imgs, f"src{k}.jpg.src")
        Image.fromarray(np.ascontiguousarray(synth.make_image(k, W, H)[:, :, ::-1])).save(fn, format="JPEG", quality=92)
        distinct.append(fn)
    with open(os.path.join(d, "odo.txt"), "w") as fh:
        for k, (t, p_) in enumerate(zip(ts, poses)):
            fh.write(synth.odometry_line(t, p_))
            shutil.copyfile(distinct[k % 8], os.path.join(imgs, "%f.jpg" % t))
    exes = {"branch": exe}
    if a.parent:
        exes["parent"] = os.path.join(a.parent, "pointcloudprocessor_amd/host/bin/PointCloudProcessor")
    out = {"keyframes": N, "image": f"{W}x{H}", "points": n_points, "decoder_threads": 16, "runs": []}
    colours = {}
    for rep in range(a.cli_reps):
        for name, e in exes.items():
            o = os.path.join(d, f"out_{name}_{rep}") + "/"
            os.makedirs(o)
            env = dict(os.environ, PCP_CLI_TIMING=os.path.join(o, "timing.json"), PCP_DECODE_THREADS="16")
            t0 = time.perf_counter()
            p = subprocess.run([e, "-p", pcd, "-o", os.path.join(d, "odo.txt"), "-i", imgs + "/", "-t", o, "--skip_filtered_dumps", "1"],
                               capture_output=True, text=True, env=env, cwd=o)
            wall = time.perf_counter() - t0
            if p.returncode != 0:
                out["runs"].append({"tree": name, "error": p.stderr[-400:]})
                continue
            ph = json.load(open(os.path.join(o, "timing.json")))
            out["runs"].append({"tree": name, "wall_s": round(wall, 3),
                                "images_decode_and_upload_wall_s": round(ph.get("images_decode_and_upload_wall_s", 0), 3),
                                "images_decode_thread_seconds": round(ph.get("images_decode_thread_seconds", 0), 3),
                                "images_upload_calls_s": round(ph.get("images_upload_calls_s", 0), 3),
                                "images_jpeg_on_device": ph.get("images_jpeg_on_device"),
                                "images_decoded_on_host": ph.get("images_decoded_on_host"),
                                "phases_s": {k_: round(v, 4) for k_, v in ph.items()}})
            colours.setdefault(name, open(os.path.join(o, "cloudInWorldWithRGB.pcd"), "rb").read())
            shutil.rmtree(o, ignore_errors=True)
    if len(colours) == 2:
        out["colours_identical_to_parent"] = colours["branch"] == colours["parent"]
    return out


if __name__ == "__main__":
    main()
