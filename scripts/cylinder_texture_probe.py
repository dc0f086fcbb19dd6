#!/usr/bin/env python3
"""Orthophotos of unrolled maps ("Orthophotos of unrolled maps") at scale, on one MI355X.  Run it under one `timeout`.

    python scripts/cylinder_texture_probe.py [--points N] [--frames F] [--gsd G] [--scale K] [--views M] [--repeats 3] [--md FILE]

Two scenes, each coloured in one shot at 1920x1080, every kernel time the device time under PCP_K_MISC with no layer leaving the
device, two warm-up rounds, then --repeats rounds, median [min .. max]:

  room      the C3 shape (10 M points x 256 keyframes).  The coloured rows' map under the fitted planar frame, filled at R = 4, through
            pcp_ortho_texture (k_ortho_texture<false>); beside it the same rows under a cylinder's frame of the SAME raster that is
            nearly that plane -- R = 1000 m, the axis along the picture's y a kilometre in front of it, theta = 0 at column 0 --
            through pcp_ortho_texture_cyl (<true>): the same number of fine pixels and, within the 8 cm the arc bulges over 13 m,
            the same picture, in the same session.  The surface pixels and the (tile, keyframe) pairs walked are printed beside
            the times, and the time per walked pair.
  vault     a vault of R 3 over 108 degrees seen from inside and a closed pier of R 0.3 in front of it, seen from outside, the
            same number of points and keyframes (the keyframes scattered about six stations inside the vault): each structure's
            unrolled map, every has bit set, filled at R = 4, through pcp_ortho_texture_cyl.

One JSON line per measurement on stdout, progress on stderr; --md writes the same as a table.  Not collected by pytest."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def quaternion_y(deg):
    import math

    return [0.0, math.sin(math.radians(deg) / 2.0), 0.0, math.cos(math.radians(deg) / 2.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--gsd", type=float, default=0.005)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import numpy as np

    from pointcloudprocessor_amd import capi, synth

    rows = []

    def say(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    cd = synth.camera_dict("cfg")
    W, H = cd["image_width"], cd["image_height"]
    p = capi.ortho_texture_params(args.scale, args.views, True, 0.05)

    def measure(ctx, scene, case, call, frame):
        """the kernel of `call` on the live, finished map of `frame`"""
        counts = np.zeros(4, np.int64)
        dev = []
        for rep in range(2 + args.repeats):
            ctx.synchronize()
            ctx.timing_reset()
            ctx._check(call(ctx.h, capi.C.byref(p), None, None, None, None, None, capi._ptr(counts)))
            if rep >= 2:
                dev.append(ctx.timing_get(capi.K_MISC)[0])
        status = np.empty((frame.height * args.scale, frame.width * args.scale), np.uint8)
        ctx._check(call(ctx.h, capi.C.byref(p), None, None, capi._ptr(status), None, None, capi._ptr(counts)))
        surface, textured, unseen, skipped = (int(v) for v in counts)
        fh, fw = status.shape
        th, tw = -(-fh // 16), -(-fw // 16)
        pad = np.zeros((th * 16, tw * 16), bool)
        pad[:fh, :fw] = status > 0
        tiles = int(pad.reshape(th, 16, tw, 16).any(axis=(1, 3)).sum())
        walked = tiles * args.frames - skipped
        ms = statistics.median(dev)
        say(scene=scene, case=case, raster=[frame.width, frame.height], fine_pixels=fh * fw, surface=surface, textured=textured, unseen=unseen,
            tiles_with_surface=tiles, pairs_walked=walked, skipped_share=round(skipped / max(tiles * args.frames, 1), 4), kernel_ms=spread(dev),
            ns_per_fine_pixel=round(ms * 1e6 / (fh * fw), 3), us_per_walked_pair=round(ms * 1e3 / max(walked, 1), 4))

    def prepare(ctx, x, y, z, poses):
        ctx.set_camera(capi.camera_from_dict(cd))
        e = x[:0]
        ctx.upload_cloud(e, e, e)  # (the image uploads ask for a cloud)
        ctx.set_frames(poses)
        for f in range(len(poses)):
            ctx.upload_image(f, synth.make_image(f % 16, W, H))
        ctx.synchronize()
        print("images uploaded", file=sys.stderr, flush=True)
        ctx.timing_enable(True)
        ctx.upload_cloud(x, y, z)
        ctx.colorize(download=False)
        ctx.synchronize()

    say(library=os.environ.get("PCP_HIP_LIBRARY", "default"), points=args.points, frames=args.frames, gsd=args.gsd, scale=args.scale, views=args.views)
    # -- the room: a planar frame and a cylinder's frame of the same raster --------------------------------------------------------
    x, y, z, _ = synth.make_cloud(args.points, seed=synth.SEED)
    xyz = np.stack([x, y, z], axis=1)
    poses, _ = synth.make_trajectory(args.frames, seed=synth.SEED)
    with capi.Context(0) as ctx:
        prepare(ctx, x, y, z, poses)
        has = (ctx.download_result_packed() >> 24).astype(np.uint8)
        plane = capi.ortho_fit_frame_host(xyz, args.gsd, has=has, viewer=np.asarray(poses, np.float64).reshape(-1, 7)[:, :3].mean(axis=0))
        # seen from inside: e = n (outward is the viewing direction), b = u (the arc runs along the picture's x), a = v; e x b = a
        o, u, v, n = (np.array(list(getattr(plane, k)), np.float64) for k in ("o", "u", "v", "n"))
        cyl = capi.cyl_frame(dict(c=o - 1000.0 * n, a=v, e=n, b=u, radius=1000.0, gsd=args.gsd, width=plane.width, height=plane.height,
                                  d_min=plane.d_min - 1.0, d_max=plane.d_max + 1.0, side=1))
        for case, begin, frame, call in (("planar, k_ortho_texture<false>", ctx.ortho_begin, plane, ctx.lib.pcp_ortho_texture),
                                         ("cylinder of R 1000, k_ortho_texture<true>", ctx.ortho_begin_cyl, cyl, ctx.lib.pcp_ortho_texture_cyl),
                                         ("planar again", ctx.ortho_begin, plane, ctx.lib.pcp_ortho_texture)):
            begin(frame)
            ctx.ortho_add(0)
            ctx.ortho_finish(4)
            measure(ctx, "room", case, call, frame)
            ctx.ortho_end()
    del x, y, z, xyz
    # -- the vault and the pier -------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(5)
    n_vault = args.points * 4 // 5
    n_pier = args.points - n_vault
    half_arc, half_y, r_vault, r_pier, axis = np.radians(54.0), 0.76, 3.0, 0.3, np.array([-0.7, 0.0, 2.2])
    t, yy = rng.uniform(-half_arc, half_arc, n_vault), rng.uniform(-half_y, half_y, n_vault)
    r = r_vault + 0.01 * np.sin(9 * t) * np.cos(5 * yy) + rng.normal(0, 0.002, n_vault)
    vault = np.stack([r * np.sin(t), yy, r * np.cos(t)], axis=1)
    t, yy = rng.uniform(0, 2 * np.pi, n_pier), rng.uniform(-0.35, 0.35, n_pier)
    r = r_pier + 0.004 * np.sin(5 * t) + rng.normal(0, 0.001, n_pier)
    pier = axis + np.stack([r * np.sin(t), yy, r * np.cos(t)], axis=1)
    pts = np.concatenate([vault, pier]).astype(np.float32)
    stations = np.array([[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.0], [0.0, 0.0, -0.6, 0.0], [-0.8, 0.0, 0.0, 15.0], [0.9, 0.1, 0.2, -18.0],
                         [0.3, -0.1, -0.3, -6.0]])
    poses = []
    for f in range(args.frames):
        s = stations[f % 6]
        poses.append(list(s[:3] + rng.uniform(-0.2, 0.2, 3) * (f >= 6)) + quaternion_y(s[3] + rng.uniform(-10, 10) * (f >= 6)))
    poses = np.array(poses)
    a = np.array([0.0, 1.0, 0.0])
    e = np.array([-np.sin(half_arc + 0.02), 0.0, np.cos(half_arc + 0.02)])
    g = float(np.float32(args.gsd))
    frames = dict(
        vault=capi.cyl_frame(dict(c=(0.0, -0.77, 0.0), a=a, e=e, b=np.cross(a, e), radius=r_vault, gsd=args.gsd,
                                  width=int(np.ceil(2 * (half_arc + 0.02) * r_vault / g)), height=int(np.ceil(1.54 / g)), d_min=-0.1, d_max=0.1, side=1)),
        pier=capi.cyl_frame(dict(c=axis + [0.0, -0.35, 0.0], a=a, e=(0.0, 0.0, -1.0), b=-np.cross(a, np.array([0.0, 0.0, -1.0])), radius=r_pier,
                                 gsd=args.gsd, width=int(np.ceil(2 * np.pi * r_pier / g)), height=int(np.ceil(0.7 / g)), d_min=-0.05, d_max=0.05,
                                 side=-1)))
    with capi.Context(0) as ctx:
        prepare(ctx, pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy(), poses)
        words = np.full(len(pts), 0x01808080, np.uint32)
        for name, frame in frames.items():
            ctx.ortho_begin_cyl(frame)
            ctx.ortho_add_packed(words)
            ctx.ortho_finish(4)
            measure(ctx, "vault", name + ", k_ortho_texture<true>", ctx.lib.pcp_ortho_texture_cyl, frame)
            ctx.ortho_end()
    if args.md:
        with open(args.md, "w") as f:
            f.write("| scene | case | raster | fine pixels | surface | textured | pairs walked | skipped share | kernel ms | ns per fine pixel | us per walked pair |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows[1:]:
                ms = r["kernel_ms"]
                f.write(f"| {r['scene']} | {r['case']} | {r['raster'][0]} x {r['raster'][1]} | {r['fine_pixels']} | {r['surface']} | {r['textured']} | "
                        f"{r['pairs_walked']} | {r['skipped_share']} | {ms['median']} [{ms['min']} .. {ms['max']}] | {r['ns_per_fine_pixel']} | "
                        f"{r['us_per_walked_pair']} |\n")


if __name__ == "__main__":
    main()
