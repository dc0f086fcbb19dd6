"""--deviceReader 1 end to end: the ASCII map (-p) and the crop CloudSmooth reads back are parsed on the device, and every file
the command line writes, its stdout and its exit code are those of --deviceReader 0.  A run that fell back to the host reader
says so on stderr, so the identical-files cases also assert that nothing was said; the fallback cases assert that it was."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 2400, 1800  # (tests/test_cli_device_writer_gpu.py: every keyframe's _rgb-mask dump needs points in the image)
FALLBACK = "read by the host reader"


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["PointCloudProcessor"]


def _header(n, data, fields="x y z intensity", k=4):
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %d\nHEIGHT 1\n"
            "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n" % (fields, " ".join("4" * k), " ".join("F" * k), " ".join("1" * k), n, n, data)).encode()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the 40 k-point wall of tests/test_cli_device_writer_gpu.py with its map written as ASCII ('%.9g'), and variants of that
    map: one hex-float token, a short row in the middle, CRLF line ends, the same points as DATA binary"""
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("device_reader")
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
    rows4 = np.concatenate([pts, inten[:, None]], 1).astype(np.float64).tolist()
    lines = [b"%.9g %.9g %.9g %.9g" % tuple(r) for r in rows4]
    m = len(lines)
    (d / "scans.pcd").write_bytes(_header(m, "ascii") + b"\n".join(lines) + b"\n")
    (d / "crlf.pcd").write_bytes(_header(m, "ascii").replace(b"\n", b"\r\n") + b"\r\n".join(lines) + b"\r\n")
    hexed = list(lines)
    hexed[12345] = b"0x1.8p1 " + hexed[12345].split(b" ", 1)[1]
    (d / "hex.pcd").write_bytes(_header(m, "ascii") + b"\n".join(hexed) + b"\n")
    short = list(lines)
    short[20000] = b"1 2 3"
    (d / "short.pcd").write_bytes(_header(m, "ascii") + b"\n".join(short) + b"\n")
    (d / "binary.pcd").write_bytes(_header(m, "binary") + np.concatenate([pts, inten[:, None]], 1).astype("<f4").tobytes())
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


def _cli(ds, out, *extra, pcd="scans.pcd"):
    out.mkdir()
    src = str(ds) + "/"
    cmd = [_exe(), "-p", src + pcd, "-o", src + "odo.txt", "-i", src, "-m", src, "-t", str(out) + "/"]
    env = dict(os.environ, PCP_CLI_TIMING=str(out / "timing.json"))
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=out, env=env)  # (<stem>_mls.pcd goes to the working directory)


def _files(root):
    return {os.path.relpath(os.path.join(d, f), root): os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f != "timing.json"}


def _pair(ds, tmp_path, flags, pcd="scans.pcd"):
    """the same run with --deviceReader 0 and 1: same exit code, stdout and files; returns both results"""
    host = _cli(ds, tmp_path / "host", *flags, "--deviceReader", "0", pcd=pcd)
    dev = _cli(ds, tmp_path / "dev", *flags, "--deviceReader", "1", pcd=pcd)
    assert host.returncode == dev.returncode, dev.stderr[-2000:]
    assert host.stdout.replace(str(tmp_path / "host"), "") == dev.stdout.replace(str(tmp_path / "dev"), ""), "the same messages"
    a, b = _files(tmp_path / "host"), _files(tmp_path / "dev")
    assert sorted(a) == sorted(b)
    for name in sorted(a):
        with open(a[name], "rb") as fa, open(b[name], "rb") as fb:
            assert fa.read() == fb.read(), name
    assert FALLBACK not in host.stderr
    return host, dev, a


MLS = ("--enableMLS", "1", "--mlsVoxelSize", "0.004", "--mlsDilationIterations", "1")


@pytest.mark.parametrize("flags, expect", [
    (("--skip_filtered_dumps", "0"), ("scans-crop.pcd", "cloudInWorldWithRGB.pcd", "cloudInWorldWithRGBandMask.pcd")),
    (MLS + ("--skip_filtered_dumps", "1"), ("scans-crop.pcd", "scans-crop_mls.pcd", "cloudInWorldWithRGB.pcd")),
    (MLS + ("--skip_filtered_dumps", "1", "--deviceWriter", "1"), ("scans-crop.pcd", "scans-crop_mls.pcd", "cloudInWorldWithRGB.pcd")),
], ids=["one_shot_with_dumps", "mls_crop_reread", "with_device_writer"])
def test_device_reader_runs_equal_host_reader_runs(dataset, tmp_path, flags, expect):
    host, dev, files = _pair(dataset, tmp_path, flags)
    assert host.returncode == 0, host.stdout[-600:] + host.stderr[-2000:]
    assert FALLBACK not in dev.stderr, "the device reader read the files itself: " + dev.stderr[-500:]
    for name in expect:
        assert name in files and os.path.getsize(files[name]) > 100_000, name
    if flags[:2] == ("--skip_filtered_dumps", "0"):
        assert sum(n.endswith("_beforeNID.pcd") for n in files) == 6 and sum(n.endswith("_rgb-mask.pcd") for n in files) == 6
    for run in ("host", "dev"):
        with open(tmp_path / run / "timing.json") as f:
            assert "pcd_read_s" in json.load(f), run


def test_a_hex_float_token_falls_back_by_name_with_the_host_reader_s_files(dataset, tmp_path):
    host, dev, files = _pair(dataset, tmp_path, ("--skip_filtered_dumps", "1"), pcd="hex.pcd")
    assert host.returncode == 0 and "cloudInWorldWithRGB.pcd" in files
    line = [ln for ln in dev.stderr.splitlines() if FALLBACK in ln]
    assert len(line) == 1 and "hex.pcd" in line[0] and "row 12345" in line[0], dev.stderr[-500:]


def test_a_short_row_ends_the_run_as_the_host_reader_ends_it(dataset, tmp_path):
    host, dev, _ = _pair(dataset, tmp_path, ("--skip_filtered_dumps", "1"), pcd="short.pcd")
    assert host.returncode != 0 and "Couldn't read point cloud file." in host.stderr + host.stdout
    strip = lambda s: [ln for ln in s.splitlines() if FALLBACK not in ln]  # noqa: E731
    assert strip(dev.stderr) == strip(host.stderr)
    assert "short.pcd" in dev.stderr and "row 20000" in dev.stderr


def test_a_binary_map_ignores_the_flag_and_a_crlf_map_is_read_on_the_device(dataset, tmp_path):
    (tmp_path / "b").mkdir()
    (tmp_path / "c").mkdir()
    host, dev, files = _pair(dataset, tmp_path / "b", ("--skip_filtered_dumps", "1"), pcd="binary.pcd")
    assert host.returncode == 0 and FALLBACK not in dev.stderr and "cloudInWorldWithRGB.pcd" in files
    host, dev, files = _pair(dataset, tmp_path / "c", ("--skip_filtered_dumps", "1"), pcd="crlf.pcd")
    assert host.returncode == 0 and FALLBACK not in dev.stderr and "cloudInWorldWithRGB.pcd" in files


def test_device_reader_2_is_refused_as_device_writer_2_is(dataset, tmp_path):
    r = _cli(dataset, tmp_path / "r", "--deviceReader", "2")
    w = _cli(dataset, tmp_path / "w", "--deviceWriter", "2")
    assert r.returncode == w.returncode != 0
    assert "--deviceReader" in r.stderr and "invalid" in r.stderr
    assert r.stderr.replace("deviceReader", "deviceWriter") == w.stderr
    assert not [f for f in (tmp_path / "r").iterdir() if f.name != "timing.json"], "refused before anything was read or written"
