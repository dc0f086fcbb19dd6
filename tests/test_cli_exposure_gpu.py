"""--balanceExposure end to end: exposure_gains.txt holds the library path's gains, cloudInWorldWithRGB.pcd its gained colours;
0 is the run without the flag, byte for byte; the refused combinations exit as the other refusals do."""
import os
import subprocess

import numpy as np
import pytest

from _exposure_ref import K_EXPOSURE

pytestmark = pytest.mark.gpu

W, H = 1024, 750
N, F = 60000, 6


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["PointCloudProcessor"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("exposure")
    x, y, z, inten = synth.make_cloud(N, seed=9)
    n = len(x)
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
            f"COUNT 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(d / "scans.pcd", "wb") as f:
        f.write(head.encode())
        f.write(np.stack([x, y, z, inten], 1).astype("<f4").tobytes())
    poses, ts = synth.make_trajectory(F)
    images = []
    with open(d / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(ts, poses)):
            f.write(synth.odometry_line(t, p))
            im = np.clip(synth.make_image(k, W, H).astype(np.float32) * np.float32(K_EXPOSURE[k]), 0, 255).astype(np.uint8)
            images.append(im)
            with open(d / ("%f.ppm" % t), "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (W, H) + im[:, :, ::-1].tobytes())
    return dict(dir=d, x=x, y=y, z=z, poses=poses, ts=ts, images=images)


def _cli(ds, out, *extra):
    out.mkdir()
    src = str(ds["dir"]) + "/"
    return subprocess.run([_exe(), "-p", src + "scans.pcd", "-o", src + "odo.txt", "-i", src, "-t", str(out) + "/", *extra],
                          capture_output=True, text=True)


def _files(out):
    return {str(q.relative_to(out)): q.read_bytes() for q in sorted(out.rglob("*")) if q.is_file()}


def _library(ds):
    """the same run through the library: gains, packed gained colours"""
    from pointcloudprocessor_amd import capi

    cam = capi.default_camera()
    cam.image_width, cam.image_height = W, H
    with capi.Context(0) as ctx:
        ctx.set_camera(cam)
        ctx.upload_cloud(ds["x"], ds["y"], ds["z"])
        ctx.set_frames(ds["poses"])
        ctx.set_image_adjust(True)
        for f in range(F):
            ctx.upload_image(f, ds["images"][f])
        ctx.colour_reset()
        ctx.depth_pass()
        ctx.colour_pass()
        g = capi.exposure_gains(*ctx.view_pair_stats())
        ctx.set_frame_gains(g)
        ctx.colour_finalise(download=False)
        return g, ctx.download_result_packed()


def test_balanced_run_writes_the_library_gains_and_colours(dataset, tmp_path):
    base = tmp_path / "base"
    p = _cli(dataset, base)
    assert p.returncode == 0, p.stderr[-2000:]
    off = tmp_path / "off"
    p = _cli(dataset, off, "--balanceExposure", "0")
    assert p.returncode == 0, p.stderr[-2000:]
    assert _files(off) == _files(base) and "exposure_gains.txt" not in _files(base)
    on = tmp_path / "on"
    p = _cli(dataset, on, "--balanceExposure", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    a, b = _files(base), _files(on)
    # one more file, and only the final colours change: the per-keyframe dumps keep the sampled colours
    assert set(b) == set(a) | {"exposure_gains.txt"}
    for name in a:
        assert (a[name] == b[name]) == (name != "cloudInWorldWithRGB.pcd"), name
    g, w = _library(dataset)
    assert np.max(np.abs(g - 1.0)) > 0.02
    lines = b["exposure_gains.txt"].decode().split("\n")
    assert lines[-1] == "" and len(lines) == F + 1
    for k, line in enumerate(lines[:F]):
        assert line == "%f %.9g" % (dataset["ts"][k], g[k]), (k, line)
    rows = [l.split() for l in b["cloudInWorldWithRGB.pcd"].decode().split("\n") if l and l[0] in "-0123456789"]
    sel = np.nonzero(w >> 24)[0]
    assert len(rows) == len(sel) > 100
    packed = 0xFF000000 | ((w[sel] & 0xFF).astype(np.uint64) << 16) | (((w[sel] >> 8) & 0xFF).astype(np.uint64) << 8) | (
        (w[sel] >> 16) & 0xFF).astype(np.uint64)
    assert np.array_equal(np.array([int(r[3]) for r in rows], dtype=np.uint64), packed)
    xyz = np.array([[float(v) for v in r[:3]] for r in rows])
    assert np.allclose(xyz, np.stack([dataset["x"], dataset["y"], dataset["z"]], 1)[sel], rtol=6e-8)


def test_refused_combinations(dataset, tmp_path):
    for k, extra in enumerate((["--gpus", "2"], ["--streamColour", "1", "--enableMLS", "1", "--skip_filtered_dumps", "1"])):
        out = tmp_path / ("r%d" % k)
        p = _cli(dataset, out, "--balanceExposure", "1", *extra)
        assert p.returncode == 254 and "--balanceExposure 1" in p.stderr and "does not work with" in p.stderr, p.stderr
        assert not os.listdir(out)  # refused before anything is read or written
