"""--outputLeaf L / --skip_full_cloud end to end: the voxel-grid output of the command line ("Voxel-grid output").
Without the flag the run writes today's files; with it cloudInWorldWithRGB_voxel.pcd holds the rows the pipeline's reduction
returns, printed by the host writer; the file is the same with and without the full-resolution files, and the same from the
one-shot path and from --streamColour 1."""
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 1024, 750
VOXEL_RGB, VOXEL_MASK = "cloudInWorldWithRGB_voxel.pcd", "cloudInWorldWithRGBandMask_voxel.pcd"
FULL_RGB, FULL_MASK = "cloudInWorldWithRGB.pcd", "cloudInWorldWithRGBandMask.pcd"


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["PointCloudProcessor"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the scene of the streamed-colour CLI suite: a curved wall patch in view of six keyframes, stray points, far points"""
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("voxel_output")
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
    # the poses as the command line reads them back from the odometry text
    read = np.loadtxt(d / "odo.txt", dtype=np.float64, ndmin=2)[:, 1:8]
    return dict(dir=d, pts=pts, poses=read)


def _cli(ds, out, *extra, masks=False, mls=False):
    out.mkdir()
    src = str(ds["dir"]) + "/"
    cmd = [_exe(), "-p", src + "scans.pcd", "-o", src + "odo.txt", "-i", src, "-t", str(out) + "/", "--skip_filtered_dumps", "1"]
    if mls:
        cmd += ["--enableMLS", "1", "--mlsVoxelSize", "0.004", "--mlsDilationIterations", "1"]
    if masks:
        cmd += ["-m", src, "--fuseMasks", "1"]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=out)


def _files(out):
    return {str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()}


def _body(data: bytes):
    head, body = data.split(b"DATA ascii\n", 1)
    return int(re.search(rb"^POINTS (\d+)$", head, re.M).group(1)), body


def test_flag_off_writes_todays_files_and_the_voxel_file_holds_the_pipelines_rows(dataset, tmp_path):
    from pointcloudprocessor_amd import capi, pipeline, synth

    plain = _cli(dataset, tmp_path / "plain")
    assert plain.returncode == 0, plain.stderr[-2000:]
    zero = _cli(dataset, tmp_path / "zero", "--outputLeaf", "0")
    assert zero.returncode == 0, zero.stderr[-2000:]
    a, b = _files(tmp_path / "plain"), _files(tmp_path / "zero")
    assert sorted(a) == sorted(b) and a == b and FULL_RGB in a and not any("voxel" in k for k in a)
    for run in (plain, zero):
        assert "voxel output:" not in run.stdout and "Voxel-grid" not in run.stdout
    leaf = _cli(dataset, tmp_path / "leaf", "--outputLeaf", "0.05")
    assert leaf.returncode == 0, leaf.stderr[-2000:]
    c = _files(tmp_path / "leaf")
    assert sorted(c) == sorted(list(a) + [VOXEL_RGB]) and all(c[k] == a[k] for k in a), "the other files are untouched"
    # the pipeline's reduction of the same run, printed by the host writer
    eng = pipeline.HipEngine(0)
    try:
        cam = capi.default_camera()
        cam.image_width, cam.image_height = W, H
        eng.configure(cam, capi.default_cull_params())
        pts = dataset["pts"]
        eng.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
        eng.ctx.set_frames(dataset["poses"])
        eng.ctx.set_image_adjust(True)
        for k in range(len(dataset["poses"])):
            eng.ctx.upload_image(k, synth.make_image(k, W, H))
        out = pipeline.PointCloudColorizer(eng).run(download=False, output_leaf=0.05)
        assert out["rgb"] is None and set(out["voxel"]) == {"xyz", "rgb", "count", "rows"}
        vox = out["voxel"]
    finally:
        eng.close()
    points, body = _body(c[VOXEL_RGB])
    full_points, _ = _body(a[FULL_RGB])
    print("coloured rows", full_points, "voxels at 0.05:", points)
    assert points == len(vox["count"]) and 100 < points < full_points and vox["rows"] == full_points
    assert int(vox["count"].sum()) == full_points
    assert body == capi.ascii_rows_host(capi.ROWS_XYZRGB, vox["xyz"], vox["rgb"]).tobytes()
    # the same voxel file without the full-resolution files
    skip = _cli(dataset, tmp_path / "skip", "--outputLeaf", "0.05", "--skip_full_cloud", "1")
    assert skip.returncode == 0, skip.stderr[-2000:]
    d = _files(tmp_path / "skip")
    assert set(d) == (set(a) - {FULL_RGB}) | {VOXEL_RGB} and d[VOXEL_RGB] == c[VOXEL_RGB]


@pytest.mark.parametrize("masks", [False, True])
def test_streamed_and_one_shot_voxel_files_are_the_same(dataset, tmp_path, masks):
    common = ("--outputLeaf", "0.02")
    one = _cli(dataset, tmp_path / "one", *common, "--streamColour", "0", masks=masks, mls=True)
    assert one.returncode == 0, one.stderr[-2000:]
    st = _cli(dataset, tmp_path / "streamed", *common, "--streamColour", "1", "--streamChunk", "4096", masks=masks, mls=True)
    assert st.returncode == 0, st.stderr[-2000:]
    m = re.search(r"^streamed colour: (\d+) chunks, (\d+) rows, (\d+) coloured$", st.stdout, re.M)
    assert m and int(m.group(1)) >= 3, st.stdout[-2000:]
    names = (VOXEL_RGB, VOXEL_MASK) if masks else (VOXEL_RGB,)
    for name in names:
        a, b = (tmp_path / "one" / name).read_bytes(), (tmp_path / "streamed" / name).read_bytes()
        assert len(a) > 10_000 and a == b, name
    assert masks or not (tmp_path / "streamed" / VOXEL_MASK).exists()
    points, _ = _body((tmp_path / "streamed" / VOXEL_RGB).read_bytes())
    assert 1000 < points < int(m.group(3)), "fewer voxels than coloured rows"
    if masks:
        _, body = _body((tmp_path / "streamed" / VOXEL_MASK).read_bytes())
        assert len({row.split()[-1] for row in body.splitlines()}) >= 2, "more than one mean label"
        # and with --skip_full_cloud 1 the chunks' rows never leave the device: same voxel files, no full files
        skip = _cli(dataset, tmp_path / "skip", *common, "--streamColour", "1", "--streamChunk", "4096", "--skip_full_cloud", "1",
                    masks=True, mls=True)
        assert skip.returncode == 0, skip.stderr[-2000:]
        for name in names:
            assert (tmp_path / "skip" / name).read_bytes() == (tmp_path / "streamed" / name).read_bytes(), name
        assert not (tmp_path / "skip" / FULL_RGB).exists() and not (tmp_path / "skip" / FULL_MASK).exists()
        assert (tmp_path / "streamed" / FULL_RGB).exists() and (tmp_path / "streamed" / FULL_MASK).exists()
        assert not list((tmp_path / "skip").glob("*.tmp"))


def test_exposure_gains_and_colour_smoothing_enter_the_voxel_file_with_and_without_the_full_files(dataset, tmp_path):
    """--balanceExposure 1 and --smoothColorsRadius change the colour result on the device; the voxel file is made from that
    result, and --skip_full_cloud 1 (which leaves the result on the device) writes the same bytes."""
    plain = _cli(dataset, tmp_path / "plain", "--outputLeaf", "0.05")
    assert plain.returncode == 0, plain.stderr[-2000:]
    common = ("--outputLeaf", "0.05", "--balanceExposure", "1", "--smoothColorsRadius", "0.03")
    both = _cli(dataset, tmp_path / "both", *common)
    assert both.returncode == 0, both.stderr[-2000:]
    skip = _cli(dataset, tmp_path / "skip", *common, "--skip_full_cloud", "1")
    assert skip.returncode == 0, skip.stderr[-2000:]
    a, b, c = _files(tmp_path / "plain"), _files(tmp_path / "both"), _files(tmp_path / "skip")
    assert b[VOXEL_RGB] != a[VOXEL_RGB], "the gains and the smoothing change the voxel colours"
    assert b[FULL_RGB] != a[FULL_RGB]
    assert c[VOXEL_RGB] == b[VOXEL_RGB]
    assert set(c) == set(b) - {FULL_RGB} and "exposure_gains.txt" in c and c["exposure_gains.txt"] == b["exposure_gains.txt"]


@pytest.mark.parametrize("flags, needles", [
    (("--outputLeaf", "0.05", "--gpus", "2"), ("--outputLeaf", "--gpus", "voxel sums", "not built")),
    (("--skip_full_cloud", "1"), ("--skip_full_cloud 1", "--outputLeaf")),
    (("--outputLeaf", "2"), ("--outputLeaf", "invalid")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, needles):
    p = _cli(dataset, tmp_path / "out", *flags)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
