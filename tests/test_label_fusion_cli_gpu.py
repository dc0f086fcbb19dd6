"""--fuseMasks 1 end to end: cloudInWorldWithRGBandMask.pcd has the rows of cloudInWorldWithRGB.pcd with the library's fused
label per map point; --gpus 2 (rehearsed on one GPU, as the sharded CLI tests do) writes the same bytes as --gpus 1, also with
--smoothColorsRadius; --matchBack radius; a missing mask ends the run."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 2400, 1800  # the CLI keeps the reference's K (cx = 2032, cy = 1535): the image must reach the optical axis
N, F = 120_001, 5


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["PointCloudProcessor"]


def _write_pcd_binary(path, x, y, z, inten):
    n = len(x)
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
            f"COUNT 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(np.stack([x, y, z, inten], 1).astype("<f4").tobytes())


def _read_pcd_ascii(path):
    header, rows = {}, []
    with open(path) as f:
        for line in f:
            if line.startswith("DATA"):
                break
            if not line.startswith("#"):
                k, *v = line.split()
                header[k] = v
        for line in f:
            rows.append(line.split())
    return header, rows


def _gray_mask(k):
    from pointcloudprocessor_amd import synth

    g = synth.make_image(k + 100, W, H)[:, :, 2].copy()
    g[synth.make_mask(k, W, H) == 255] = 255
    return g


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("fuse")
    rng = np.random.default_rng(3)
    x, y, z, inten = synth.make_cloud(N - 4000, seed=21)
    dup = rng.choice(len(x), 4000, replace=False)  # exact duplicates: --matchBack radius has neighbours to credit
    x, y, z, inten = (np.concatenate([a, a[dup]]) for a in (x, y, z, inten))
    order = rng.permutation(len(x))
    x, y, z, inten = (np.ascontiguousarray(a[order]) for a in (x, y, z, inten))
    _write_pcd_binary(d / "scans.pcd", x, y, z, inten)
    poses, ts = synth.make_trajectory(F)
    images, masks = [], []
    with open(d / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(ts, poses)):
            f.write(synth.odometry_line(t, p))
            images.append(synth.make_image(k, W, H))
            masks.append(_gray_mask(k))
            with open(d / ("%f.ppm" % t), "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (W, H) + images[k][:, :, ::-1].tobytes())
            with open(d / ("%f.pgm" % t), "wb") as g:
                g.write(b"P5\n%d %d\n255\n" % (W, H) + masks[k].tobytes())
    return dict(dir=d, x=x, y=y, z=z, poses=poses, ts=ts, images=images, masks=masks)


def _cli(ds, out, *extra, gpus="1"):
    out.mkdir()
    env = dict(os.environ, PCP_MULTI_REHEARSAL="1")
    src = str(ds["dir"]) + "/"
    p = subprocess.run([_exe(), "-p", src + "scans.pcd", "-o", src + "odo.txt", "-i", src, "-m", src, "-t", str(out) + "/",
                        "--gpus", gpus, *extra], capture_output=True, text=True, env=env)
    return p


def _files(out):
    return {str(q.relative_to(out)): q.read_bytes() for q in sorted(out.rglob("*.pcd"))}


def _library(ds, match_mode, smooth=0.0):
    """the same run through the library: packed colours, has and the fused labels"""
    from pointcloudprocessor_amd import capi

    cam = capi.default_camera()
    cam.image_width, cam.image_height = W, H
    cull = capi.default_cull_params()
    cull.match_mode = match_mode
    with capi.Context(0) as ctx:
        ctx.set_camera(cam, cull)
        ctx.upload_cloud(ds["x"], ds["y"], ds["z"])
        ctx.set_frames(ds["poses"])
        ctx.set_image_adjust(True)
        for f in range(F):
            ctx.upload_image(f, ds["images"][f])
            ctx.upload_mask(f, ds["masks"][f])
        ctx.set_label_fusion(True)
        ctx.colorize(download=False)
        if smooth:
            ctx.colour_smooth_local(smooth)
        w = ctx.download_result_packed()
        lab = ctx.colour_labels()
    return w, lab


def _check_against_library(ds, out, match_mode, smooth=0.0):
    w, lab = _library(ds, match_mode, smooth)
    sel = np.nonzero(w >> 24)[0]
    h_rgb, r_rgb = _read_pcd_ascii(out / "cloudInWorldWithRGB.pcd")
    h_m, r_m = _read_pcd_ascii(out / "cloudInWorldWithRGBandMask.pcd")
    assert h_m["FIELDS"] == ["x", "y", "z", "rgb", "segmentMask"]
    assert len(r_rgb) == len(r_m) == len(sel) > 1000
    # exactly the rows of the RGB file: the map point's x y z and the same rgb
    assert [r[:4] for r in r_m] == [r[:4] for r in r_rgb]
    xyz = np.array([[float(v) for v in r[:3]] for r in r_m])
    assert np.allclose(xyz, np.stack([ds["x"], ds["y"], ds["z"]], 1)[sel], rtol=6e-8)
    packed = 0xFF000000 | ((w[sel] & 0xFF).astype(np.uint64) << 16) | (((w[sel] >> 8) & 0xFF).astype(np.uint64) << 8) | (
        (w[sel] >> 16) & 0xFF).astype(np.uint64)
    assert np.array_equal(np.array([int(r[3]) for r in r_m], dtype=np.uint64), packed)  # no (255,0,0) override
    got = np.array([int(r[4]) for r in r_m])
    assert np.array_equal(got, lab["label"][sel])
    assert ((got > 0) & (got < 255)).sum() > 500 and (got == 255).sum() > 10
    return lab


def test_fused_mask_file_has_the_rgb_rows_and_the_library_labels(dataset, tmp_path):
    from pointcloudprocessor_amd import capi

    base = tmp_path / "base"
    p = _cli(dataset, base)
    assert p.returncode == 0, p.stderr[-2000:]
    one = tmp_path / "one"
    p = _cli(dataset, one, "--fuseMasks", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    a, b = _files(base), _files(one)
    # only the mask file changes: the per-keyframe dumps are still written, the colours are the same
    assert set(a) == set(b) and len(a) == 3 + 2 * F
    for name in a:
        assert (a[name] == b[name]) == (name != "cloudInWorldWithRGBandMask.pcd"), name
    _check_against_library(dataset, one, capi.MATCH_ROUNDTRIP)
    # --gpus 2 == --gpus 1, byte for byte
    two = tmp_path / "two"
    p = _cli(dataset, two, "--fuseMasks", "1", gpus="2")
    assert p.returncode == 0, p.stderr[-2000:]
    c = _files(two)
    assert set(c) == set(b)
    for name in b:
        assert b[name] == c[name], name
    # --skip_filtered_dumps 1: no per-keyframe loop at all, the same two map files
    skip = tmp_path / "skip"
    p = _cli(dataset, skip, "--fuseMasks", "1", "--skip_filtered_dumps", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    d = _files(skip)
    assert sorted(d) == ["cloudInWorldWithRGB.pcd", "cloudInWorldWithRGBandMask.pcd", "scans-crop.pcd"]
    for name in d:
        assert d[name] == b[name], name


def test_fused_with_local_colour_smoothing_over_two_gpus(dataset, tmp_path):
    from pointcloudprocessor_amd import capi

    outs = {}
    for gpus in ("1", "2"):
        out = tmp_path / ("g" + gpus)
        p = _cli(dataset, out, "--fuseMasks", "1", "--smoothColorsRadius", "0.1", "--skip_filtered_dumps", "1", gpus=gpus)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[gpus] = _files(out)
    assert set(outs["1"]) == set(outs["2"])
    for name in outs["1"]:
        assert outs["1"][name] == outs["2"][name], name
    _check_against_library(dataset, tmp_path / "g1", capi.MATCH_ROUNDTRIP, smooth=0.1)


def test_fused_with_radius_match_back(dataset, tmp_path):
    from pointcloudprocessor_amd import capi

    out = tmp_path / "radius"
    p = _cli(dataset, out, "--fuseMasks", "1", "--matchBack", "radius", "--skip_filtered_dumps", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    lab = _check_against_library(dataset, out, capi.MATCH_RADIUS)
    rt = _library(dataset, capi.MATCH_ROUNDTRIP)[1]
    assert (lab["views"] != rt["views"]).sum() > 100  # the duplicates were credited with their twins' samples


def test_missing_mask_ends_the_run(dataset, tmp_path):
    import shutil

    src = tmp_path / "in"
    shutil.copytree(dataset["dir"], src)
    gone = src / ("%f.pgm" % dataset["ts"][2])
    os.remove(gone)
    out = tmp_path / "out"
    out.mkdir()
    s = str(src) + "/"
    p = subprocess.run([_exe(), "-p", s + "scans.pcd", "-o", s + "odo.txt", "-i", s, "-m", s, "-t", str(out) + "/",
                        "--fuseMasks", "1"], capture_output=True, text=True)
    assert p.returncode == 254
    assert "Failed to read image from: " + s + ("%f.png" % dataset["ts"][2]) in p.stderr
    assert not (out / "cloudInWorldWithRGBandMask.pcd").exists()
