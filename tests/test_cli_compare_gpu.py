"""--compareMap base.pcd end to end ("Map comparison"): distance.npy, lod.npy and status.npy hold, byte for byte, what
PointCloudColorizer.compare_map returns for the same map, base and keyframes; compare.json carries the stats; with --orthoMap 1
change.npy and change_status.npy are ortho_change_layers of the written index layer; every other output file is byte for byte
the file of a run without the flag; the refusals name the flags."""
import json
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 1024, 750
FLAGS = ("--normalRadius", "0.5", "--compareRadius", "0.3", "--compareDepth", "0.3", "--compareMinPoints", "3")
PARAMS = dict(normal_radius=0.5, radius=0.3, half_length=0.3, min_points=3)


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["PointCloudProcessor"]


def _write_pcd(path, pts, inten):
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
            f"COUNT 1 1 1 1\nWIDTH {len(pts)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(pts)}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(np.concatenate([pts, inten[:, None]], 1).astype("<f4").tobytes())


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, small_scene):
    """small_scene's 20 k points as the map; the base is a copy with one flat patch of 1 m radius moved 5 mm along the patch's
    own normal (the smallest eigenvector of its covariance)"""
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("compare_cli")
    s = small_scene
    pts = np.stack([s["x"], s["y"], s["z"]], axis=1).astype(np.float32)
    flat = []
    for i in range(40):  # the flattest neighbourhood among the first points: one that lies on a single wall
        near = np.linalg.norm(pts.astype(np.float64) - pts[i].astype(np.float64), axis=1) < 1.0
        val, vec = np.linalg.eigh(np.cov(pts[near].astype(np.float64).T))
        flat.append((val[0] / val[1] if near.sum() >= 100 else np.inf, i, near, vec))
    _, centre, patch, vec = min(flat, key=lambda f: f[0])
    base = pts.copy()
    base[patch] = (pts[patch].astype(np.float64) + 0.005 * vec[:, 0]).astype(np.float32)
    inten = np.random.default_rng(3).random(len(pts), dtype=np.float32)
    _write_pcd(d / "scans.pcd", pts, inten)
    _write_pcd(d / "base.pcd", base, inten)
    with open(d / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(s["ts"], s["poses"])):
            f.write(synth.odometry_line(t, p))
            with open(d / ("%f.ppm" % t), "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (W, H) + synth.make_image(k, W, H)[:, :, ::-1].tobytes())
    read = np.loadtxt(d / "odo.txt", dtype=np.float64, ndmin=2)  # the poses as the command line reads them back
    return dict(dir=d, pts=pts, base=base, patch=patch, centre=centre, poses=read[:, 1:8], ts=read[:, 0])


def _cli(ds, out, *extra):
    out.mkdir()
    src = str(ds["dir"]) + "/"
    cmd = [_exe(), "-p", src + "scans.pcd", "-o", src + "odo.txt", "-i", src, "-t", str(out) + "/", "--skip_filtered_dumps", "1"]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=out)


def _files(out):
    return {str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()}


def _library(ds):
    from pointcloudprocessor_amd import capi, pipeline

    eng = pipeline.HipEngine(0)
    try:
        cam = capi.default_camera()
        cam.image_width, cam.image_height = W, H
        eng.configure(cam, capi.default_cull_params())
        pts = ds["pts"]
        eng.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
        eng.set_keyframes(ds["poses"])
        return pipeline.PointCloudColorizer(eng).compare_map(ds["base"], **PARAMS)
    finally:
        eng.close()


def test_files_hold_the_librarys_comparison_and_nothing_else_changes(dataset, tmp_path):
    from pointcloudprocessor_amd import pipeline

    ds = dataset
    base = str(ds["dir"] / "base.pcd")
    plain = _cli(ds, tmp_path / "plain")
    assert plain.returncode == 0, plain.stderr[-2000:]
    run = _cli(ds, tmp_path / "run", "--compareMap", base, *FLAGS)
    assert run.returncode == 0, run.stderr[-2000:]
    a, c = _files(tmp_path / "plain"), _files(tmp_path / "run")
    new = ["compare/distance.npy", "compare/lod.npy", "compare/status.npy", "compare/compare.json"]
    assert not any(k.startswith("compare/") for k in a) and sorted(c) == sorted(list(a) + new)
    assert all(c[k] == a[k] for k in a), "every other output file is byte for byte the same"
    want = _library(ds)
    got = {k: np.load(tmp_path / "run" / "compare" / f"{k}.npy") for k in ("distance", "lod", "status")}
    assert got["distance"].dtype == np.dtype("<f4") and got["lod"].dtype == np.dtype("<f4") and got["status"].dtype == np.dtype("|u1")
    for k in got:
        assert got[k].shape == (len(ds["pts"]),) and got[k].tobytes() == want[k].tobytes(), k
    meta = json.loads((tmp_path / "run" / "compare" / "compare.json").read_text())
    assert meta["stats"] == [int(v) for v in want["stats"]] and meta["base"] == len(ds["base"]) and meta["points"] == len(ds["pts"])
    third = float("%.9g" % np.float32(0.3))
    assert (meta["min_points"], meta["orient_mode"], meta["radius"], meta["half_length"], meta["reg_error"]) == (3, 1, third, third, 0.0)
    sig = want["distance"][want["status"] >= 4].astype(np.float64)
    assert meta["significant"] == len(sig) == meta["positive"] + meta["negative"]
    assert meta["significant_min"] == float("%.9g" % sig.min(initial=np.inf)) if len(sig) else meta["significant_min"] == 0.0
    assert meta["significant_max"] == float("%.9g" % sig.max(initial=-np.inf)) if len(sig) else meta["significant_max"] == 0.0
    assert abs(meta["significant_mean"] - (sig.mean() if len(sig) else 0.0)) <= 1e-9
    assert f"{meta['measured']} of {meta['core']} core points measured" in run.stdout
    # The patch moved 5 mm as a whole.  A measured point whose whole search sphere (0.43 m) lies inside the patch sees every base
    # candidate moved by the same vector, whose component along a unit direction is at most 5 mm: 0 < |distance| <= 5 mm (and the
    # roundings, far below 2 um); a point further than patch + sphere from its centre sees the same rows in both epochs: exactly 0.
    from_centre = np.linalg.norm(ds["pts"].astype(np.float64) - ds["pts"][ds["centre"]].astype(np.float64), axis=1)
    moved = (from_centre < 1.0 - 0.43) & (want["status"] >= 3)
    still = (from_centre > 1.0 + 0.43) & (want["status"] >= 3)
    size = np.abs(want["distance"][moved].astype(np.float64))
    print("patch", int(ds["patch"].sum()), "inner measured", int(moved.sum()), "median |d|", np.median(size), "largest", size.max(),
          "elsewhere", int(still.sum()), "significant", len(sig))
    assert moved.sum() > 20 and (size > 0).all() and (size <= 0.005 + 2e-6).all() and np.median(size) > 0.0025
    assert still.sum() > 10000 and not want["distance"][still].any() and (want["status"][still] == 3).all()

    # with --orthoMap 1: the change layers beside the map's layers
    both = _cli(ds, tmp_path / "both", "--compareMap", base, *FLAGS, "--orthoMap", "1", "--orthoGsd", "0.05")
    assert both.returncode == 0, both.stderr[-2000:]
    only = _cli(ds, tmp_path / "only", "--orthoMap", "1", "--orthoGsd", "0.05")
    assert only.returncode == 0, only.stderr[-2000:]
    e, o = _files(tmp_path / "both"), _files(tmp_path / "only")
    assert sorted(e) == sorted(list(o) + new + ["ortho/change.npy", "ortho/change_status.npy"]) and all(e[k] == o[k] for k in o)
    assert all(e[k] == c[k] for k in new)
    index = np.load(tmp_path / "both" / "ortho" / "ortho_index.npy")
    layers = pipeline.ortho_change_layers(index, want["distance"], want["status"])
    change, status = np.load(tmp_path / "both" / "ortho" / "change.npy"), np.load(tmp_path / "both" / "ortho" / "change_status.npy")
    assert change.dtype == np.dtype("<f4") and status.dtype == np.dtype("|u1") and change.shape == index.shape == status.shape
    assert change.tobytes() == layers["change"].tobytes() and status.tobytes() == layers["change_status"].tobytes()
    drawn = index != 0xFFFFFFFF  # (the map draws the coloured points only: few of this scene under the default camera)
    assert drawn.any() and np.array_equal(status[drawn], want["status"][index[drawn]])
    assert not change[index == 0xFFFFFFFF].any() and not status[index == 0xFFFFFFFF].any()


@pytest.mark.parametrize("flags, needles", [
    (("--gpus", "2"), ("--compareMap", "--gpus", "index shard", "not built")),
    (("--enableMLS", "1"), ("--compareMap", "--enableMLS 1", "not built")),
    (("--enableMLS", "1", "--streamColour", "1"), ("--compareMap", "--streamColour 1", "chunk")),
    (("--normalRadius", "0"), ("--compareMap", "--normalRadius 0")),
    (("--compareRadius", "0.004"), ("--compareRadius", "invalid")),
    (("--compareMinPoints", "1"), ("--compareMinPoints", "invalid")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, needles):
    p = _cli(dataset, tmp_path / "out", "--compareMap", str(dataset["dir"] / "base.pcd"), *flags)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
