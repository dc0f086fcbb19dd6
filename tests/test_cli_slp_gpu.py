"""--enableMLS 1 --mlsUpsampling slp through the command line: the smoothed crop against pcp_cloud_smooth on the crop the
run wrote, with a non-default disk (--mlsUpsamplingRadius / --mlsUpsamplingStep), and --gpus 3 (three contexts on the
one GPU, PCP_MULTI_REHEARSAL=1) byte-identical to --gpus 1: MultiCloudSmooth runs the SAMPLE_LOCAL_PLANE chain on the
first GPU."""
import os
import subprocess

import numpy as np
import pytest

from test_cli import _exe, _read_pcd_ascii, _write_pcd_binary

pytestmark = pytest.mark.gpu


def test_cli_slp_matches_library_and_gpus_agree(tmp_path):
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import capi, synth

    W, H = 640, 480
    rng = np.random.default_rng(17)
    poses, ts = synth.make_trajectory(3, spacing=0.12)
    n = 8000
    p0 = poses[0, :3]
    R0 = npo.quat_to_rot(*poses[0, 3:7])
    a, b = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    depth = 1.7 + 0.04 * np.cos(4.0 * b) + rng.normal(0, 1e-3, n)
    wall = p0 + a[:, None] * R0[:, 0] + b[:, None] * R0[:, 1] + depth[:, None] * R0[:, 2]
    stray = rng.uniform(-1.0, 1.0, (100, 3)) + p0 + 0.5 * R0[:, 2]
    pts = np.concatenate([wall, stray]).astype(np.float32)
    _write_pcd_binary(tmp_path / "scans.pcd", pts[:, 0], pts[:, 1], pts[:, 2], rng.random(len(pts), dtype=np.float32))
    with open(tmp_path / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(ts, poses)):
            f.write(synth.odometry_line(t, p))
            img = synth.make_image(k, W, H)
            with open(tmp_path / ("%f.ppm" % t), "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (W, H) + img[:, :, ::-1].tobytes())
    radius, step = 0.03, 0.0075
    outs = {}
    for gpus in (1, 3):
        out = tmp_path / f"g{gpus}"
        out.mkdir()
        p = subprocess.run([_exe(), "-p", str(tmp_path / "scans.pcd"), "-o", str(tmp_path / "odo.txt"), "-i", str(tmp_path) + "/",
                            "-t", str(out) + "/", "--enableMLS", "1", "--mlsUpsampling", "slp", "--mlsUpsamplingRadius",
                            str(radius), "--mlsUpsamplingStep", str(step), "--gpus", str(gpus), "--skip_filtered_dumps", "1"],
                           capture_output=True, text=True, cwd=out, env=dict(os.environ, PCP_MULTI_REHEARSAL="1"))
        assert p.returncode == 0, p.stderr[-2000:]
        outs[gpus] = out
    # --gpus 3 writes what --gpus 1 writes, byte for byte
    files = sorted(f for f in os.listdir(outs[1]) if f.endswith(".pcd"))
    assert "scans-crop_mls.pcd" in files and files == sorted(f for f in os.listdir(outs[3]) if f.endswith(".pcd"))
    for f in files:
        assert (outs[1] / f).read_bytes() == (outs[3] / f).read_bytes(), f
    # the smoothed crop is pcp_cloud_smooth(SAMPLE_LOCAL_PLANE) on the crop the run wrote (and re-read, cloudSmooth.cpp:92)
    _, crop = _read_pcd_ascii(outs[1] / "scans-crop.pcd")
    crop = np.array(crop, dtype=np.float64)[:, :3].astype(np.float32)
    ctx = capi.Context(0)
    try:
        ctx.upload_cloud(crop[:, 0].copy(), crop[:, 1].copy(), crop[:, 2].copy())
        ctx.set_mls_local_plane(radius, step)
        mp = capi.default_mls_params()
        mp.upsampling = capi.UPSAMPLING_SAMPLE_LOCAL_PLANE
        m = ctx.cloud_smooth(mp)
        got = ctx.mls_fetch(m)
    finally:
        ctx.close()
    T = len(capi.mls_local_plane_samples(radius, step)[0])
    _, rows = _read_pcd_ascii(outs[1] / "scans-crop_mls.pcd")
    rows = np.array(rows, dtype=np.float64)
    assert len(rows) == m and m > 20 * T
    assert np.abs(rows[:, 0:3] - got["xyz"]).max() <= 1e-6 * max(1.0, np.abs(got["xyz"]).max())
    assert np.abs(rows[:, 3:6] - got["normal"]).max() <= 1e-6
    np.testing.assert_allclose(rows[:, 6], got["curvature"], rtol=1e-5, atol=1e-9)
