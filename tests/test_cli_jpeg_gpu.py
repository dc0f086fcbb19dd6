"""The command line with its keyframe JPEGs reconstructed on the device (pcp_upload_image_jpeg): a mix of JPEG kinds, and a
PNG named .jpg that takes the host decoder, at an image size that reaches the reference's optical axis.  The colours equal
the oracle's from Pillow-decoded pixels, the timing report counts both paths, and the --gpus 2 rehearsal writes the same
bytes as --gpus 1."""
import json
import os
import subprocess

import numpy as np
import pytest

from test_cli import _exe, _read_pcd_ascii, _write_pcd_binary

pytestmark = pytest.mark.gpu


def test_cli_device_jpeg_matches_oracle_and_sharded_run(tmp_path, oracle):
    from PIL import Image

    from pointcloudprocessor_amd import synth

    W, H = 2400, 1800  # the CLI keeps the reference's K (cx = 2032, cy = 1535): the image must reach the optical axis
    x, y, z, inten = synth.make_cloud(80_000, seed=13)
    _write_pcd_binary(tmp_path / "scans.pcd", x, y, z, inten)
    poses, ts = synth.make_trajectory(6)  # every pose a keyframe
    kinds = [dict(quality=92), dict(quality=90, subsampling=0), "grey", dict(quality=85, optimize=True),
             dict(quality=88, subsampling=2, restart_marker_blocks=5), "png"]
    imgs = {}
    with open(tmp_path / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(ts, poses)):
            f.write(synth.odometry_line(t, p))
            rgb = synth.make_image(k, W, H)[:, :, ::-1]
            path = tmp_path / ("%f.jpg" % t)
            if kinds[k] == "grey":
                Image.fromarray(np.ascontiguousarray(rgb[:, :, 1])).save(path, format="JPEG", quality=90)
            elif kinds[k] == "png":
                Image.fromarray(rgb).save(path, format="PNG")
            else:
                Image.fromarray(rgb).save(path, format="JPEG", **kinds[k])
            imgs[k] = np.ascontiguousarray(np.array(Image.open(path).convert("RGB"))[:, :, ::-1])
            Image.fromarray(synth.make_mask(k, W, H)).save(tmp_path / ("%f.png" % t))
    outs = {}
    for gpus in ("1", "2"):
        d = tmp_path / ("out" + gpus)
        d.mkdir()
        env = dict(os.environ, PCP_MULTI_REHEARSAL="1", PCP_CLI_TIMING=str(d / "timing.json"))
        p = subprocess.run([_exe(), "-p", str(tmp_path / "scans.pcd"), "-o", str(tmp_path / "odo.txt"), "-i", str(tmp_path) + "/",
                            "-m", str(tmp_path) + "/", "-t", str(d) + "/", "--gpus", gpus], capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        timing = json.loads((d / "timing.json").read_text())
        assert timing["images_jpeg_on_device"] == 5 and timing["images_decoded_on_host"] == 1, timing
        assert "images_decode_thread_seconds" in timing and "images_decode_and_upload_wall_s" in timing
        files = sorted(str(q.relative_to(d)) for q in d.rglob("*.pcd"))
        outs[gpus] = {name: (d / name).read_bytes() for name in files}
    assert set(outs["1"]) == set(outs["2"]) and len(outs["1"]) == 3 + 2 * 6
    for name in outs["1"]:
        assert outs["1"][name] == outs["2"][name], name
    # the colours against the oracle, from Pillow's pixels after generateColorMap's HSV round trip
    cam = oracle.default_camera()
    cam.image_width, cam.image_height = W, H
    cp = oracle.default_cull_params()
    adj = [oracle.hsv_round_trip(imgs[k]) for k in range(6)]
    ref = oracle.colorize(cam, cp, x, y, z, poses, adj, threads=8)
    header, rows = _read_pcd_ascii(tmp_path / "out1" / "cloudInWorldWithRGB.pcd")
    sel = np.nonzero(ref["has"])[0]
    assert len(rows) == len(sel) > 1000
    got_rgb = np.array([int(r[3]) for r in rows], dtype=np.uint64)
    packed = (0xFF000000 | (ref["rgb"][sel, 0].astype(np.uint64) << 16) | (ref["rgb"][sel, 1].astype(np.uint64) << 8)
              | ref["rgb"][sel, 2].astype(np.uint64))
    assert np.array_equal(got_rgb, packed)
    # the per-keyframe dumps sample the same pixels
    for k in range(6):
        vis = oracle.frame_visible(cam, cp, poses[k], x, y, z, adj[k], synth.make_mask(k, W, H))
        _, r3 = _read_pcd_ascii(tmp_path / "out1" / "filtered_pcd" / ("%f_rgb-mask.pcd" % ts[k]))
        assert len(r3) == len(vis["index"])
        if len(r3):
            want = (vis["rgb"][:, 0].astype(np.uint64) << 16) | (vis["rgb"][:, 1].astype(np.uint64) << 8) | vis["rgb"][:, 2]
            assert np.array_equal(np.array([int(r[3]) for r in r3], dtype=np.uint64) & 0xFFFFFF, want)
