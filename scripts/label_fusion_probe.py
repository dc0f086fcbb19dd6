#!/usr/bin/env python3
"""Cost of the fused segmentation labels (pcp_set_label_fusion); writes one JSON file.  Not collected by pytest.

    python scripts/label_fusion_probe.py [out.json] [n_points] [n_frames]

  step               C3-size colourise steps (10 M points x 256 keyframes @1920x1080, images and masks resident): pcp_colorize
                     without download, fusion off and on ALTERNATING in one process, timed with a host clock around the call
                     and a device synchronisation; per mode the median / min of the timed steps and the PCP_K_COLOUR kernel
                     time per step.  The label form's only extra traffic is one 4-byte store per point per result.
  labels_download    pcp_colour_labels (unpack kernel + three n-byte copies to pageable host memory), median
  cli                host/bin/PointCloudProcessor with masks on a cli_e2e-size dataset (1 M points, 32 keyframes
                     @1920x1080, tmpfs), --fuseMasks 0 and 1 alternating, twice each: wall time and the mask phases the
                     binary reports (PCP_CLI_TIMING)
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudprocessor_amd import capi, host_build, synth  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "label_fusion_probe.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
F = int(sys.argv[3]) if len(sys.argv) > 3 else 256
WARM, STEPS = 2, 10


def gray_mask(f, W, H):
    g = synth.make_image(f + 100, W, H)[:, :, 0].copy()
    g[synth.make_mask(f, W, H) == 255] = 255
    return g


def step_leg():
    cd = synth.camera_dict("cfg")
    W, H = cd["image_width"], cd["image_height"]
    x, y, z, _ = synth.make_cloud(N)
    poses, _ = synth.make_trajectory(F)
    res = {"points": N, "keyframes": F, "image": f"{W}x{H}", "timed_steps_per_mode": STEPS}
    with capi.Context(0) as ctx:
        ctx.set_camera(capi.camera_from_dict(cd))
        ctx.upload_cloud(x, y, z)
        ctx.set_frames(poses)
        for f in range(F):
            ctx.upload_image(f, synth.make_image(f, W, H))
            ctx.upload_mask(f, gray_mask(f, W, H))
        times = {False: [], True: []}
        kernel = {False: 0.0, True: 0.0}
        for it in range(WARM + STEPS):
            for on in (False, True):
                ctx.set_label_fusion(on)
                ctx.synchronize()
                if it >= WARM:
                    ctx.timing_reset()
                    ctx.timing_enable(True)
                t0 = time.perf_counter()
                ctx.colorize(download=False)
                ctx.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if it >= WARM:
                    times[on].append(dt)
                    kernel[on] += ctx.timing_get(capi.K_COLOUR)[0]
                    ctx.timing_enable(False)
        for on, name in ((False, "fusion_off"), (True, "fusion_on")):
            res[name] = {"step_ms_median": round(float(np.median(times[on])), 3), "step_ms_min": round(float(np.min(times[on])), 3),
                         "step_ms_all": [round(t, 3) for t in times[on]],
                         "colour_kernels_ms_per_step": round(kernel[on] / STEPS, 3)}
        res["extra_store_bytes_per_result"] = 4 * N
        dl = []
        for _ in range(5):
            t0 = time.perf_counter()
            lab = ctx.colour_labels()
            dl.append((time.perf_counter() - t0) * 1e3)
        res["labels_download_ms_median"] = round(float(np.median(dl)), 3)
        res["labels_download_ms_all"] = [round(t, 3) for t in dl]
        res["labelled_points"] = int((lab["views"] > 0).sum())
    return res


def cli_leg(n_points=1_000_000, n_frames=32, W=1920, H=1080):
    from PIL import Image

    exe = host_build.build()["PointCloudProcessor"]
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    d = tempfile.mkdtemp(prefix="pcp_label_probe_", dir=base)
    res = {"points": n_points, "keyframes": n_frames, "image": f"{W}x{H}", "filesystem": base}
    try:
        x, y, z, inten = synth.make_cloud(n_points)
        pcd = os.path.join(d, "scans.pcd")
        hdr = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\n"
               f"TYPE F F F F\nCOUNT 1 1 1 1\nWIDTH {n_points}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n_points}\nDATA binary\n")
        with open(pcd, "wb") as fh:
            fh.write(hdr.encode())
            fh.write(np.stack([x, y, z, inten], 1).astype(np.float32).tobytes())
        poses, ts = synth.make_trajectory(n_frames)
        with open(os.path.join(d, "odo.txt"), "w") as fh:
            for k, (t, p_) in enumerate(zip(ts, poses)):
                fh.write(synth.odometry_line(t, p_))
                Image.fromarray(synth.make_image(k, W, H)[:, :, ::-1]).save(os.path.join(d, "%f.jpg" % t), quality=92)
                Image.fromarray(gray_mask(k, W, H)).save(os.path.join(d, "%f.png" % t))
        keys = ("frame_visible_gpu_s", "rgb_mask_dumps_write_ascii_s", "colourise_gpu_s", "labels_gpu_s", "mask_pcd_rows_s",
                "final_pcd_write_ascii_s", "total")
        for rep in range(2):
            for fuse in (0, 1):
                out = os.path.join(d, f"out{fuse}_{rep}") + "/"
                os.makedirs(out)
                env = dict(os.environ, PCP_CLI_TIMING=os.path.join(out, "timing.json"))
                t1 = time.perf_counter()
                p = subprocess.run([exe, "-p", pcd, "-o", os.path.join(d, "odo.txt"), "-i", d + "/", "-m", d + "/", "-t", out,
                                    "--fuseMasks", str(fuse)], capture_output=True, text=True, env=env, cwd=out)
                wall = time.perf_counter() - t1
                name = f"fuse_masks_{fuse}"
                if p.returncode != 0:
                    res[name] = {"error": f"exit {p.returncode}: {p.stderr[-300:]}"}
                    continue
                with open(os.path.join(out, "timing.json")) as fh:
                    phases = json.load(fh)
                mask_file = os.path.getsize(os.path.join(out, "cloudInWorldWithRGBandMask.pcd"))
                shutil.rmtree(out, ignore_errors=True)
                run = {"wall_s": round(wall, 3), "mask_file_bytes": int(mask_file),
                       "phases_s": {k: round(phases.get(k, 0.0), 4) for k in keys}}
                run["mask_phase_s"] = round(sum(phases.get(k, 0.0) for k in ("frame_visible_gpu_s", "rgb_mask_dumps_write_ascii_s",
                                                                             "labels_gpu_s", "mask_pcd_rows_s")), 4)
                res.setdefault(name, []).append(run)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return res


def main():
    res = {"what": "fused segmentation labels: colourise step with fusion off / on, label download, CLI mask phases",
           "step": step_leg()}
    with open(OUT, "w") as fh:  # (the first leg is kept if the second fails)
        json.dump(res, fh, indent=1)
    res["cli"] = cli_leg()
    with open(OUT, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
