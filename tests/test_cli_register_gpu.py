"""--compareRegister 1 end to end ("Map registration"): registration.json and base_transform.txt hold what
PointCloudColorizer.register_base returns for the same map, base and flags, and the comparison's arrays are those of compare_map
after it; a planted 4 mm shift of the base is taken out before the comparison; a run without the flag writes the files it wrote
before; the refusals name the flags."""
import hashlib
import json
import pathlib
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 1024, 750
FLAGS = ("--normalRadius", "0.5", "--compareRadius", "0.3", "--compareDepth", "0.3", "--compareMinPoints", "3")
PARAMS = dict(normal_radius=0.5, radius=0.3, half_length=0.3, min_points=3)
REG_FLAGS = ("--compareRegister", "1", "--registerRadius", "0.3", "--registerMaxDistance", "0.1", "--registerStride", "2", "--registerIterations", "15")
REG_PARAMS = dict(match_radius=0.3, max_plane_distance=0.1, sample_stride=2, max_iterations=15)
COMPARE_FILES = ["compare/distance.npy", "compare/lod.npy", "compare/status.npy", "compare/compare.json"]
COMPARE_KEYS = ["base", "points", "radius", "half_length", "reg_error", "min_points", "normal_radius", "orient_mode", "viewer", "stats", "core",
                "measured", "positive", "negative", "no_counterpart", "too_few_own", "most_candidates", "significant", "significant_mean",
                "significant_min", "significant_max"]


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


def write_dataset(d, s):
    """small_scene's 20 k points as the map; same.pcd is a copy of it, shifted.pcd that copy moved rigidly by 4 mm and 0.05
    degrees about the cloud's middle"""
    import _register_ref as ref
    from pointcloudprocessor_amd import synth

    pts = np.stack([s["x"], s["y"], s["z"]], axis=1).astype(np.float32)
    mid = pts.astype(np.float64).mean(axis=0)
    R = ref.rodrigues(np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8]) * np.radians(0.05))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mid - R @ mid + np.array([0.6, 0.64, -0.48]) * 0.004
    shifted = ref.moved(pts, np.linalg.inv(T))
    inten = np.random.default_rng(3).random(len(pts), dtype=np.float32)
    _write_pcd(d / "scans.pcd", pts, inten)
    _write_pcd(d / "same.pcd", pts, inten)
    _write_pcd(d / "shifted.pcd", shifted, inten)
    with open(d / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(s["ts"], s["poses"])):
            f.write(synth.odometry_line(t, p))
            with open(d / ("%f.ppm" % t), "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (W, H) + synth.make_image(k, W, H)[:, :, ::-1].tobytes())
    read = np.loadtxt(d / "odo.txt", dtype=np.float64, ndmin=2)  # the poses as the command line reads them back
    return dict(dir=d, pts=pts, shifted=shifted, T_true=T, poses=read[:, 1:8], ts=read[:, 0])


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, small_scene):
    return write_dataset(tmp_path_factory.mktemp("register_cli"), small_scene)


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
        col = pipeline.PointCloudColorizer(eng)
        reg = col.register_base(ds["shifted"], normal_radius=0.5, **REG_PARAMS)
        return reg, col.compare_map(None, **PARAMS)
    finally:
        eng.close()


def test_files_hold_the_librarys_registration_and_the_shift_is_taken_out(dataset, tmp_path):
    import _register_ref as ref

    ds = dataset
    src = str(ds["dir"]) + "/"
    same = _cli(ds, tmp_path / "same", "--compareMap", src + "same.pcd", *FLAGS)
    assert same.returncode == 0, same.stderr[-2000:]
    off = _cli(ds, tmp_path / "off", "--compareMap", src + "shifted.pcd", *FLAGS)
    assert off.returncode == 0, off.stderr[-2000:]
    run = _cli(ds, tmp_path / "run", "--compareMap", src + "shifted.pcd", *FLAGS, *REG_FLAGS)
    assert run.returncode == 0, run.stderr[-2000:]
    a, b, c = _files(tmp_path / "same"), _files(tmp_path / "off"), _files(tmp_path / "run")
    # without the flag: the files of before, compare.json with the keys of before
    assert sorted(k for k in a if k.startswith("compare/")) == sorted(COMPARE_FILES) and sorted(a) == sorted(b)
    assert list(json.loads(a["compare/compare.json"])) == COMPARE_KEYS == list(json.loads(c["compare/compare.json"]))
    # ... and their bytes: tests/golden/register_cli_flagless.json holds compare.json and the SHA-256 of the three arrays as the
    # parent commit's program wrote them for this map and shifted.pcd (made once with that program, on the device)
    golden = json.loads((pathlib.Path(__file__).parent / "golden" / "register_cli_flagless.json").read_text())
    assert b["compare/compare.json"].decode() == golden["compare.json"]
    assert {k: hashlib.sha256(b[k]).hexdigest() for k in COMPARE_FILES[:3]} == golden["sha256"]
    new = ["compare/registration.json", "compare/base_transform.txt"]
    assert sorted(c) == sorted(list(b) + new)
    assert all(c[k] == b[k] for k in b if not k.startswith("compare/")), "every other output file is byte for byte the same"

    reg, want = _library(ds)
    meta = json.loads(c["compare/registration.json"])
    assert np.array(meta["T"], np.float64).tobytes() == reg["T"].tobytes()
    assert np.loadtxt(tmp_path / "run" / "compare" / "base_transform.txt", dtype=np.float64).tobytes() == reg["T"].tobytes()
    assert np.array(meta["log"], np.float64).reshape(-1, 5).tobytes() == reg["log"].tobytes()
    assert (meta["status"], meta["iterations"], meta["pairs"], meta["dof"], meta["rms"]) == (reg["status"], reg["iterations"], reg["pairs"], reg["dof"], reg["rms"])
    assert (meta["sample_stride"], meta["max_iterations"], meta["min_pairs"], meta["base"]) == (2, 15, 100, len(ds["shifted"]))
    assert meta["match_radius"] == float(np.float32(0.3)) and meta["max_plane_distance"] == float(np.float32(0.1))
    assert f"after {reg['iterations']} iterations" in run.stdout and "--compareRegError" in run.stdout
    got = {k: np.load(tmp_path / "run" / "compare" / f"{k}.npy") for k in ("distance", "lod", "status")}
    for k in got:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert json.loads(c["compare/compare.json"])["stats"] == [int(v) for v in want["stats"]]

    # the planted motion is found, and the comparison after it is as quiet as that against the unshifted copy
    assert reg["status"] == ref.CONVERGED and reg["dof"] == 6
    err = ref.pose_error(reg["T"], ds["T_true"], ds["pts"].astype(np.float64).mean(axis=0))

    def share(out):
        st = np.load(tmp_path / out / "compare" / "status.npy")
        return float((st >= 4).sum()) / max(1, int((st >= 3).sum()))

    print("pose error", err, "rms", reg["rms"], "iterations", reg["iterations"], "significant: same", share("same"), "shifted", share("off"),
          "registered", share("run"))
    assert err[0] < 1e-3 and err[1] < 2e-4
    assert share("run") <= share("same") + 0.05
    assert share("off") > share("run")


@pytest.mark.parametrize("flags, needles", [
    (("--compareRegister", "1"), ("--compareRegister 1", "needs '--compareMap'")),
    (("--compareMap", "B", "--registerStride", "3"), ("--registerStride", "needs '--compareRegister 1'")),
    (("--compareMap", "B", "--compareRegister", "1", "--gpus", "2"), ("--compareRegister 1", "--gpus", "index shard", "not built")),
    (("--compareMap", "B", "--compareRegister", "1", "--enableMLS", "1"), ("--compareRegister 1", "--enableMLS 1", "not built")),
    (("--compareMap", "B", "--compareRegister", "1", "--enableMLS", "1", "--streamColour", "1"), ("--compareRegister 1", "--streamColour 1", "chunk")),
    (("--compareMap", "B", "--compareRegister", "1", "--registerRadius", "0.004"), ("--registerRadius", "invalid")),
    (("--compareMap", "B", "--compareRegister", "1", "--registerMaxDistance", "0.2"), ("--registerMaxDistance", "invalid", "--registerRadius")),
    (("--compareMap", "B", "--compareRegister", "1", "--registerIterations", "0"), ("--registerIterations", "invalid")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, needles):
    flags = [str(dataset["dir"] / "shifted.pcd") if f == "B" else f for f in flags]
    p = _cli(dataset, tmp_path / "out", *flags)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
