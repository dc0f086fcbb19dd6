"""--orthoDefects 1 end to end ("Surface defects on ortho maps"), on a scene of its own: a wall with one dent (a smooth
bump of 12 mm over a radius of 0.15 m, away from the keyframes) and a closed pier of R 0.4 with one dent of 12 mm towards its
axis, 1 mm of noise, both dents where the keyframes look (the command line's camera is the 4096 x 3000 sensor's and a 1024 x 750
test image is its upper left corner, 12 x 9 degrees: only what lies there is coloured and drawn).  The run writes
ortho_defect_dev.npy, ortho_defect_class.npy, ortho_defect_region.npy and defects.json beside the other layers of every
ortho/facet_<row>/, planar and unrolled, and of ortho/ for the whole map.  The wall's directory must hold a hollow at the dent's
place and of its depth, the pier's a hollow of the dent's depth; the files are, bit for bit, what capi.ortho_defects_host gives
for the directory's own depth and status layers (the device is compared with that twin in test_ortho_defects_gpu.py), and
defects.json holds the parameters, the counts and the rows with the metres derived from them; without the flag every file is
byte for byte what it was; the refusals name the flags."""
import json

import numpy as np
import pytest

import test_cli_geometry_gpu as geometry_cli

pytestmark = pytest.mark.gpu

W, H = 1024, 750
NEW = ["ortho_defect_dev.npy", "ortho_defect_class.npy", "ortho_defect_region.npy", "defects.json"]
REQUEST = dict(threshold=0.004, window=0, refine=False, min_support=1, min_pixels=10, classes=3)
FLAGS = ("--orthoDefects", "1", "--defectThreshold", "0.004", "--defectMinPixels", "10")
WHOLE = dict(threshold=0.0015, window=3, refine=True, min_support=2, min_pixels=2, classes=1)
WHOLE_FLAGS = ("--orthoDefects", "1", "--defectThreshold", "0.0015", "--defectWindow", "3", "--defectRefine", "1", "--defectMinSupport", "2",
               "--defectMinPixels", "2", "--defectClasses", "hollow")
N_WALL, N_PIER = 24000, 24000
# in the first keyframe's axes (right, down, forward)
WALL_Z, DENT_XY, DENT_A, DENT_H = 2.9, (-0.92, -0.70), 0.15, 0.012
R_PIER, PIER_AXIS = 0.4, (0.0, 2.7)  # the axis runs down through (x, z)
PIER_DENT_Y, PIER_DENT_ARC, PIER_DENT_HALF_Y = -0.5, 0.12, 0.12


def _bump(r):
    """1 at 0, 0 from 1 on, smooth"""
    return np.where(r < 1.0, 0.5 * (1.0 + np.cos(np.pi * np.minimum(r, 1.0))), 0.0)


def scene_points(p0, R0, seed=43):
    rng = np.random.default_rng(seed)
    noise = lambda n: 1e-3 * rng.normal(size=n)  # noqa: E731
    x, y = rng.uniform(-1.5, -0.45, N_WALL), rng.uniform(-1.2, -0.2, N_WALL)
    wall = np.stack([x, y, WALL_Z + DENT_H * _bump(np.hypot(x - DENT_XY[0], y - DENT_XY[1]) / DENT_A) + noise(N_WALL)], axis=1)
    t, y = rng.uniform(-np.pi, np.pi, N_PIER), rng.uniform(-1.6, 0.0, N_PIER)  # t = 0 faces the keyframes (towards -z)
    rho = R_PIER - DENT_H * _bump(np.hypot(R_PIER * t / PIER_DENT_ARC, (y - PIER_DENT_Y) / PIER_DENT_HALF_Y)) + noise(N_PIER)
    pier = np.stack([PIER_AXIS[0] + rho * np.sin(t), y, PIER_AXIS[1] - rho * np.cos(t)], axis=1)
    return (p0 + np.concatenate([wall, pier]) @ R0.T).astype(np.float32)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("defects_cli")
    poses, ts = synth.make_trajectory(4, spacing=0.12)
    p0, R0 = poses[0, :3], npo.quat_to_rot(*poses[0, 3:7])
    pts = scene_points(p0, R0)
    inten = np.random.default_rng(42).random(len(pts), dtype=np.float32)
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
    dent_world = p0 + np.array([DENT_XY[0], DENT_XY[1], WALL_Z]) @ R0.T
    return dict(dir=d, pts=pts, dent_world=dent_world)


def _g(v):
    return float("%.9g" % v)


def _check_directory(d, request):
    """the four files of one directory against the host twin on the directory's own layers; returns the counts"""
    from pointcloudprocessor_amd import capi

    depth, status = np.load(d / "ortho_depth.npy"), np.load(d / "ortho_status.npy")
    want = capi.ortho_defects_host(depth, status, **request)
    for name, key, descr in (("ortho_defect_dev", "dev", "<i4"), ("ortho_defect_class", "cls", "|u1"), ("ortho_defect_region", "region", "<i4")):
        got = np.load(d / f"{name}.npy")
        assert got.dtype == np.dtype(descr) and got.shape == depth.shape and got.tobytes() == want[key].tobytes(), (str(d), name)
    meta, rec = json.loads((d / "ortho_frame.json").read_text()), json.loads((d / "defects.json").read_text())
    g = float(np.float32(meta["gsd"]))
    assert (rec["threshold"], rec["window"], rec["refine"], rec["min_support"], rec["min_pixels"], rec["classes"]) == \
        (_g(np.float32(request["threshold"])), request["window"], int(request["refine"]), request["min_support"], request["min_pixels"], request["classes"])
    assert rec["gsd"] == _g(g) and (rec["width"], rec["height"]) == (meta["width"], meta["height"]) and rec["counts"] == [int(v) for v in want["out"]]
    assert len(rec["regions"]) == len(want["rows"])
    w = meta["width"]
    for k, (item, row) in enumerate(zip(rec["regions"], want["rows"])):
        row = [int(v) for v in row]
        px = float(row[1])
        assert item["id"] == k + 1 and item["row"] == row and item["kind"] == ("hollow" if row[0] == 1 else "bulge") and item["pixels"] == row[1]
        assert item["area_m2"] == _g(px * g * g) and item["volume_m3"] == _g(row[3] * 2.0 ** -20 * g * g) and item["depth_m"] == _g(row[4] * 2.0 ** -20)
        assert item["depth_px"] == [row[5] % w, row[5] // w] and item["box_px"] == [row[6], row[8], row[7], row[9]]
        assert item["centroid_px"] == [_g(row[10] / px), _g(row[11] / px)] and item["measured_fraction"] == _g(row[2] / px)
        assert item["open_pixels"] == row[12] and item["first_pass_pixels"] == row[14]
    return want["out"]


def test_files_of_every_facet_directory(dataset, tmp_path):
    ds = dataset
    common = ("--skip_filtered_dumps", "1", "--facets", "1", "--facetCylinders", "1", "--orthoMap", "1", "--orthoFrame", "facets", "--orthoGsd", "0.02",
              "--orthoFill", "2")
    plain = geometry_cli._cli(ds, tmp_path / "plain", *common)
    assert plain.returncode == 0, plain.stderr[-2000:]
    off = geometry_cli._cli(ds, tmp_path / "off", *common, "--orthoDefects", "0")
    assert off.returncode == 0, off.stderr[-2000:]
    run = geometry_cli._cli(ds, tmp_path / "run", *common, *FLAGS)
    assert run.returncode == 0, run.stderr[-2000:]
    a, b, c = (geometry_cli._files(tmp_path / k) for k in ("plain", "off", "run"))
    assert a == b, "without the flag every file is what it was"
    dirs = sorted({k.rsplit("/", 1)[0] for k in a if k.startswith("ortho/facet_")})
    kinds = [json.loads(a[d + "/ortho_frame.json"]).get("kind", "plane") for d in dirs]
    assert "plane" in kinds and "cylinder" in kinds, kinds
    assert sorted(c) == sorted(list(a) + [f"{d}/{name}" for d in dirs for name in NEW])
    assert all(c[k] == a[k] for k in a), "every other output file is byte for byte the same"
    found = {}
    for d, kind in zip(dirs, kinds):
        out = _check_directory(tmp_path / "run" / d, REQUEST)
        rec = json.loads(c[d + "/defects.json"])
        print(d, kind, dict(zip(("kept", "dropped", "hollow", "bulge", "unsupported", "refused", "first_pass", "surface"), out)),
              [(r["kind"], r["pixels"], r["depth_m"]) for r in rec["regions"]])
        found[kind] = (json.loads(c[d + "/ortho_frame.json"]), rec["regions"])
    assert len(dirs) == 2 and run.stdout.count("Surface defects saved to:") == 2
    # the wall: one hollow, at the dent's place and of its depth (the fitted plane lies within a millimetre of the wall)
    f, regions = found["plane"]
    assert regions and all(r["kind"] == "hollow" for r in regions)
    regions = sorted(regions, key=lambda r: -r["pixels"])
    col, row = regions[0]["centroid_px"]
    world = np.array(f["o"]) + (col + 0.5) * f["gsd"] * np.array(f["u"]) + (row + 0.5) * f["gsd"] * np.array(f["v"])
    offset = world - dataset["dent_world"]
    assert np.linalg.norm(offset - np.dot(offset, f["n"]) * np.array(f["n"])) < 0.04
    assert abs(regions[0]["depth_m"] - DENT_H) < 0.003
    radius = DENT_A * np.arccos(2 * REQUEST["threshold"] / DENT_H - 1.0) / np.pi  # where the bump exceeds the threshold
    assert abs(regions[0]["area_m2"] - np.pi * radius ** 2) < 0.35 * np.pi * radius ** 2
    # the pier, seen from outside: one hollow of the dent's depth (the dent pulls the fitted cylinder by a millimetre or two)
    f, regions = found["cylinder"]
    assert f["side"] == -1 and regions and all(r["kind"] == "hollow" for r in regions)
    regions = sorted(regions, key=lambda r: -r["pixels"])
    assert abs(regions[0]["depth_m"] - DENT_H) < 0.004 and regions[0]["pixels"] >= 15


def test_files_of_the_whole_map(dataset, tmp_path):
    run = geometry_cli._cli(dataset, tmp_path / "run", "--skip_filtered_dumps", "1", "--orthoMap", "1", "--orthoGsd", "0.02", "--orthoFill", "1",
                            *WHOLE_FLAGS)
    assert run.returncode == 0, run.stderr[-2000:]
    files = geometry_cli._files(tmp_path / "run")
    assert all(f"ortho/{name}" in files for name in NEW)
    out = _check_directory(tmp_path / "run" / "ortho", WHOLE)
    assert out[7] >= 300 and out[3] == 0  # (bulges are masked out)


@pytest.mark.parametrize("flags, needles", [
    (("--orthoDefects", "1"), ("--orthoDefects 1", "--orthoMap 1")),
    (("--orthoMap", "1", "--defectWindow", "5"), ("--defectWindow", "--orthoDefects 1")),
    (("--orthoMap", "1", "--defectClasses", "hollow"), ("--defectClasses", "--orthoDefects 1")),
    (("--orthoMap", "1", "--orthoDefects", "1", "--defectRefine", "1"), ("--defectRefine 1", "--defectWindow")),
    (("--orthoMap", "1", "--orthoDefects", "1", "--defectThreshold", "2"), ("--defectThreshold", "2^-20")),
    (("--orthoMap", "1", "--orthoDefects", "1", "--defectWindow", "1025"), ("--defectWindow", "0..1024")),
    (("--orthoMap", "1", "--orthoDefects", "1", "--defectMinPixels", "0"), ("--defectMinPixels", "1 or more")),
    (("--orthoMap", "1", "--orthoDefects", "1", "--defectClasses", "dents"), ("--defectClasses", "hollow, bulge or both")),
    (("--orthoMap", "1", "--orthoDefects", "1", "--gpus", "2"), ("--gpus",)),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, needles):
    p = geometry_cli._cli(dataset, tmp_path / "out", *flags)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
