"""--crackMaps 1 / --crackThreshold t end to end ("Mask distance maps"): the .npy files of the command line load
with numpy and hold the library's CPU form of the mask file the run read, bit for bit; every other output file is byte for
byte the file of a run without the flag; without --mask_image_folder and with --gpus 2 the run is refused with the reason."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 1024, 750
KINDS = ("edt2", "nearest")


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["PointCloudProcessor"]


def _mask(k):
    """three discs of 255 (synth.make_mask), a band of 100 across them, 0 elsewhere: thresholds 0 and 128 differ"""
    from pointcloudprocessor_amd import synth

    m = synth.make_mask(k, W, H)
    m[300 + 20 * k:340 + 20 * k, 100:900][m[300 + 20 * k:340 + 20 * k, 100:900] == 0] = 100
    return m


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """a wall patch in view of four keyframes with an image and a mask each"""
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("crack_cli")
    rng = np.random.default_rng(34)
    poses, ts = synth.make_trajectory(4, spacing=0.12)
    n = 20_000
    p0 = poses[0, :3]
    R0 = npo.quat_to_rot(*poses[0, 3:7])  # camera -> world
    a, b = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    depth = 1.9 + 0.05 * np.sin(3.0 * a)
    pts = (p0 + a[:, None] * R0[:, 0] + b[:, None] * R0[:, 1] + depth[:, None] * R0[:, 2]).astype(np.float32)
    inten = rng.random(len(pts), dtype=np.float32)
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
            f"COUNT 1 1 1 1\nWIDTH {len(pts)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(pts)}\nDATA binary\n")
    with open(d / "scans.pcd", "wb") as f:
        f.write(head.encode())
        f.write(np.concatenate([pts, inten[:, None]], 1).astype("<f4").tobytes())
    masks = []
    with open(d / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(ts, poses)):
            f.write(synth.odometry_line(t, p))
            masks.append(_mask(k))
            with open(d / ("%f.ppm" % t), "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (W, H) + synth.make_image(k, W, H)[:, :, ::-1].tobytes())
            with open(d / ("%f.pgm" % t), "wb") as g:
                g.write(b"P5\n%d %d\n255\n" % (W, H) + masks[k].tobytes())
    read = np.loadtxt(d / "odo.txt", dtype=np.float64, ndmin=2)
    return dict(dir=d, ts=read[:, 0], masks=masks)


def _cli(ds, out, *extra, masks=True, timing=None):
    out.mkdir()
    env = dict(os.environ, PCP_CLI_TIMING=str(timing)) if timing else None
    src = str(ds["dir"]) + "/"
    cmd = [_exe(), "-p", src + "scans.pcd", "-o", src + "odo.txt", "-i", src, "-t", str(out) + "/"]
    if masks:
        cmd += ["-m", src]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=out, env=env)


def _files(out):
    return {str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()}


def test_npy_files_hold_the_host_form_and_nothing_else_changes(dataset, tmp_path):
    from pointcloudprocessor_amd import capi

    plain = _cli(dataset, tmp_path / "plain", "--crackMaps", "0", "--crackThreshold", "9")
    assert plain.returncode == 0, plain.stderr[-2000:]
    maps = _cli(dataset, tmp_path / "maps", "--crackMaps", "1", timing=tmp_path / "phases.json")
    assert maps.returncode == 0, maps.stderr[-2000:]
    high = _cli(dataset, tmp_path / "high", "--crackMaps", "1", "--crackThreshold", "128", "--geometryMaps", "1", "--normalRadius", "0")
    assert high.returncode == 0, high.stderr[-2000:]
    a, c, e = _files(tmp_path / "plain"), _files(tmp_path / "maps"), _files(tmp_path / "high")
    assert not any(k.startswith("crack_maps/") for k in a)
    stems = ["crack_maps/" + "%f" % t for t in dataset["ts"]]
    new = sorted(f"{s}_{kind}.npy" for s in stems for kind in KINDS)
    assert sorted(c) == sorted(list(a) + new) and len(new) == 2 * len(dataset["masks"])
    assert all(c[k] == a[k] for k in a), "every other output file is byte for byte the same"
    assert all(e[k] == a[k] for k in a) and any(k.startswith("geometry_maps/") for k in e)
    differ = 0
    for k, stem in enumerate(stems):
        for out, files, t in (("maps", c, 0), ("high", e, 128)):
            want = capi.mask_edt_host(dataset["masks"][k], t)
            d2 = np.load(tmp_path / out / f"{stem}_edt2.npy")
            nearest = np.load(tmp_path / out / f"{stem}_nearest.npy")
            assert d2.dtype == np.dtype("<u4") and d2.shape == (H, W) and d2.flags.c_contiguous
            assert nearest.dtype == np.dtype("<i4") and nearest.shape == (H, W)
            assert files[f"{stem}_edt2.npy"][:8] == b"\x93NUMPY\x01\x00"
            assert d2.tobytes() == want["d2"].tobytes() and nearest.tobytes() == want["nearest"].tobytes(), (k, t)
            assert d2.any() and not d2.all()
        differ += c[f"{stem}_edt2.npy"] != e[f"{stem}_edt2.npy"]
        assert f"{stem.split('/')[1]}_edt2.npy" in maps.stdout
    assert differ == len(stems), "the band of 100 is foreground at threshold 0 and background at 128"
    phases = json.loads((tmp_path / "phases.json").read_text())  # the binary's own split
    assert phases["crack_maps_gpu_s"] > 0 and phases["crack_maps_write_s"] > 0


@pytest.mark.parametrize("flags, masks, needles", [
    (("--crackMaps", "1"), False, ("--crackMaps 1", "--mask_image_folder")),
    (("--crackMaps", "1", "--gpus", "2"), True, ("--crackMaps 1", "--gpus", "index shards")),
    (("--crackMaps", "1", "--crackThreshold", "256"), True, ("--crackThreshold", "invalid")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, masks, needles):
    p = _cli(dataset, tmp_path / "out", *flags, masks=masks)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
