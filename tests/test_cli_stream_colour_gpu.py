"""--enableMLS 1 --streamColour 1 end to end: the smoothing chain's chunks are coloured on the device one by one, and
scans-crop_mls.pcd, cloudInWorldWithRGB.pcd and cloudInWorldWithRGBandMask.pcd (--fuseMasks 1) are byte for byte the files of
the --streamColour 0 run of the same inputs.  Every flag combination that needs the whole smoothed cloud is refused by name."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 1024, 750
OUTPUTS = ("scans-crop_mls.pcd", "cloudInWorldWithRGB.pcd", "cloudInWorldWithRGBandMask.pcd")


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["PointCloudProcessor"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the scene of test_cli_enable_mls_end_to_end (a curved wall patch in view of six keyframes, stray points, points
    outside the crop box), with masks"""
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("stream_colour")
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


def _cli(ds, out, *extra, masks=True):
    out.mkdir()
    src = str(ds) + "/"
    cmd = [_exe(), "-p", src + "scans.pcd", "-o", src + "odo.txt", "-i", src, "-t", str(out) + "/", "--enableMLS", "1",
           "--mlsVoxelSize", "0.004", "--mlsDilationIterations", "1"]
    if masks:
        cmd += ["-m", src]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=out)  # (<stem>_mls.pcd goes to the working directory)


def test_streamed_files_are_the_one_shot_files(dataset, tmp_path):
    common = ("--fuseMasks", "1", "--skip_filtered_dumps", "1")
    one = _cli(dataset, tmp_path / "one", *common, "--streamColour", "0")
    assert one.returncode == 0, one.stderr[-2000:]
    st = _cli(dataset, tmp_path / "streamed", *common, "--streamColour", "1", "--streamChunk", "4096")
    assert st.returncode == 0, st.stderr[-2000:]
    m = re.search(r"^streamed colour: (\d+) chunks, (\d+) rows, (\d+) coloured$", st.stdout, re.M)
    assert m, st.stdout[-2000:]
    chunks, rows, coloured = (int(v) for v in m.groups())
    print("streamed colour:", chunks, "chunks,", rows, "rows,", coloured, "coloured")
    assert chunks >= 4 and "streamed colour" not in one.stdout
    for name in OUTPUTS:
        a, b = (tmp_path / "one" / name).read_bytes(), (tmp_path / "streamed" / name).read_bytes()
        assert len(a) > 100_000, name
        assert a == b, name
    points = lambda name: int(re.search(rb"^POINTS (\d+)$", (tmp_path / "streamed" / name).read_bytes()[:400], re.M).group(1))  # noqa: E731
    assert points(OUTPUTS[0]) == rows and points(OUTPUTS[1]) == points(OUTPUTS[2]) == coloured and 0 < coloured <= rows
    assert not list((tmp_path / "streamed").glob("*.tmp")), "no temporary body file is left behind"


@pytest.mark.parametrize("flags, masks, names", [
    (("--skip_filtered_dumps", "0"), False, "--skip_filtered_dumps 0"),
    (("--skip_filtered_dumps", "1", "--enableNIDOptimize", "1"), False, "--enableNIDOptimize 1"),
    (("--skip_filtered_dumps", "1", "--gpus", "2"), False, "--gpus"),
    (("--skip_filtered_dumps", "1", "--cull", "hpr"), False, "--cull hpr"),
    (("--skip_filtered_dumps", "1", "--matchBack", "radius"), False, "--matchBack radius"),
    (("--skip_filtered_dumps", "1", "--smoothColorsRadius", "0.05"), False, "--smoothColorsRadius"),
    (("--skip_filtered_dumps", "1"), True, "--fuseMasks 1"),
    (("--skip_filtered_dumps", "1", "--mlsUpsampling", "none"), False, "--mlsUpsampling"),
    (("--skip_filtered_dumps", "1", "--mlsUpsampling", "slp"), False, "--mlsUpsampling"),
])
def test_streamed_mode_refuses_what_needs_the_whole_cloud(dataset, tmp_path, flags, masks, names):
    p = _cli(dataset, tmp_path / "out", "--streamColour", "1", *flags, masks=masks)
    assert p.returncode != 0
    assert "--streamColour 1" in p.stderr and names in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
