"""--deviceWriter 1 end to end: every ASCII PCD the command line writes -- scans-crop.pcd, scans-crop_mls.pcd, the per-keyframe
_beforeNID.pcd / _rgb-mask.pcd dumps, cloudInWorldWithRGB.pcd, cloudInWorldWithRGBandMask.pcd -- is byte for byte the file of
the --deviceWriter 0 run, one-shot and streamed; --gpus N > 1 is refused by name before anything is read or written."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 2400, 1800  # the CLI keeps the reference's K (cx = 2032, cy = 1535): every keyframe's _rgb-mask dump needs points in the image
MAIN = ("scans-crop.pcd", "scans-crop_mls.pcd", "cloudInWorldWithRGB.pcd", "cloudInWorldWithRGBandMask.pcd")


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["PointCloudProcessor"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the scene of tests/test_cli_stream_colour_gpu.py: a curved 40 k-point wall in view of six keyframes, stray points, points
    outside the crop box, masks -- with images that reach the optical axis, so that every keyframe colours some points (a
    keyframe without any ends the run at its _rgb-mask dump with the writer's empty-cloud exception, as the reference does)"""
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("device_writer")
    rng = np.random.default_rng(21)
    poses, ts = synth.make_trajectory(6, spacing=0.12)
    n = 40_000
    p0 = poses[0, :3]
    R0 = npo.quat_to_rot(*poses[0, 3:7])  # camera -> world
    a, b = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    depth = 1.9 + 0.05 * np.sin(3.0 * a) + rng.normal(0, 1e-3, n)
    wall = p0 + a[:, None] * R0[:, 0] + b[:, None] * R0[:, 1] + depth[:, None] * R0[:, 2]
    stray = rng.uniform(-1.2, 1.2, (300, 3)) + p0 + 0.5 * R0[:, 2]
    far = rng.uniform(20, 30, (50, 3))
    pts = np.concatenate([wall, stray, far]).astype(np.float32)
    inten = rng.random(len(pts), dtype=np.float32)
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
            f"COUNT 1 1 1 1\nWIDTH {len(pts)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(pts)}\nDATA binary\n")
    with open(d / "scans.pcd", "wb") as f:
        f.write(head.encode())
        f.write(np.concatenate([pts, inten[:, None]], 1).astype("<f4").tobytes())
    with open(d / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(ts, poses)):
            f.write(synth.odometry_line(t, p))
            with open(d / ("%f.ppm" % t), "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (W, H) + synth.make_image(k, W, H)[:, :, ::-1].tobytes())
            gray = synth.make_image(k + 100, W, H)[:, :, 2].copy()
            gray[synth.make_mask(k, W, H) == 255] = 255
            with open(d / ("%f.pgm" % t), "wb") as g:
                g.write(b"P5\n%d %d\n255\n" % (W, H) + gray.tobytes())
    return d


def _cli(ds, out, *extra):
    out.mkdir()
    src = str(ds) + "/"
    cmd = [_exe(), "-p", src + "scans.pcd", "-o", src + "odo.txt", "-i", src, "-m", src, "-t", str(out) + "/", "--enableMLS", "1",
           "--mlsVoxelSize", "0.004", "--mlsDilationIterations", "1"]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=out)  # (<stem>_mls.pcd goes to the working directory)


def _files(root):
    return {os.path.relpath(os.path.join(d, f), root): os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs}


@pytest.mark.parametrize("flags, dumps", [
    (("--skip_filtered_dumps", "0"), True),
    (("--skip_filtered_dumps", "0", "--fuseMasks", "1"), True),
    (("--streamColour", "1", "--streamChunk", "4096", "--fuseMasks", "1", "--skip_filtered_dumps", "1"), False),
], ids=["one_shot_with_dumps", "fused_masks", "streamed"])
def test_device_writer_files_are_the_host_writer_files(dataset, tmp_path, flags, dumps):
    host = _cli(dataset, tmp_path / "host", *flags, "--deviceWriter", "0")
    assert host.returncode == 0, host.stdout[-600:] + host.stderr[-2000:]
    dev = _cli(dataset, tmp_path / "dev", *flags, "--deviceWriter", "1")
    assert dev.returncode == 0, dev.stdout[-600:] + dev.stderr[-2000:]
    assert host.stdout.replace(str(tmp_path / "host"), "") == dev.stdout.replace(str(tmp_path / "dev"), ""), "the same messages"
    a, b = _files(tmp_path / "host"), _files(tmp_path / "dev")
    assert sorted(a) == sorted(b)
    for name in MAIN:
        assert name in a and os.path.getsize(a[name]) > 100_000, name
    if dumps:
        assert sum(n.endswith("_beforeNID.pcd") for n in a) == 6 and sum(n.endswith("_rgb-mask.pcd") for n in a) == 6
    for name in sorted(a):
        with open(a[name], "rb") as fa, open(b[name], "rb") as fb:
            assert fa.read() == fb.read(), name
    assert not [n for n in b if n.endswith(".tmp")], "no temporary body file is left behind"


def test_device_writer_refuses_several_gpus(dataset, tmp_path):
    p = _cli(dataset, tmp_path / "out", "--deviceWriter", "1", "--gpus", "2")
    assert p.returncode != 0
    assert "--deviceWriter 1" in p.stderr and "--gpus" in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
