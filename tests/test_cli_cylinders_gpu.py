"""--facetCylinders 1 end to end, and the pipeline's cylinders=True beneath it ("Cylindrical facets"): a wall, a
pier (closed, R 0.4), a vault (half cylinder, R 1, the keyframes inside it) and a sphere are facets of kind 1 / 2 / 2 / 0;
--orthoMap 1 --orthoFrame facets writes one directory per planar and per cylindrical facet and none for the sphere, whose
layers are, bit for bit, ortho_maps_by_facet's; facets.json without the flag is byte for byte the file of a run that never
knew it; the refusals name the flags."""
import json

import numpy as np
import pytest

import test_cli_geometry_gpu as geometry_cli

pytestmark = pytest.mark.gpu

W, H = 1024, 750
LAYERS = (("ortho_rgb", "rgb", "|u1"), ("ortho_depth", "depth", "<f4"), ("ortho_index", "index", "<u4"), ("ortho_status", "status", "|u1"))
ORTHO = ["ortho_rgb.npy", "ortho_depth.npy", "ortho_index.npy", "ortho_status.npy", "ortho_frame.json"]
FACET = dict(link_radius=0.1, angle_deg=10.0, plane_tol=0.01, max_curvature=0.02, min_points=1000)
GSD = 0.02
CYL_KEYS = ("c", "a", "e", "b", "radius", "gsd", "width", "height", "d_min", "d_max", "side")
N_WALL, N_PIER, N_VAULT, N_SPHERE = 12000, 12000, 16000, 6000


def scene_points(p0, R0, seed=41):
    """in the first keyframe's axes (right, down, forward): a wall at depth 2.9, a pier of R 0.4 about a vertical axis at depth
    2.3, a vault of R 1 about the forward axis over the keyframes, a sphere of R 0.35; 1 mm of noise along the normals"""
    rng = np.random.default_rng(seed)
    noise = lambda n: 1e-3 * rng.normal(size=n)
    a, b = rng.uniform(-0.9, 0.9, N_WALL), rng.uniform(-0.6, 0.9, N_WALL)
    wall = np.stack([a, b, 2.9 + noise(N_WALL)], axis=1)
    t, h, r = rng.uniform(0, 2 * np.pi, N_PIER), rng.uniform(-0.3, 0.9, N_PIER), 0.4 + noise(N_PIER)
    pier = np.stack([0.3 + r * np.cos(t), h, 2.3 + r * np.sin(t)], axis=1)
    t, h, r = rng.uniform(0, np.pi, N_VAULT), rng.uniform(1.0, 2.6, N_VAULT), 1.0 + noise(N_VAULT)
    vault = np.stack([r * np.cos(t), 0.2 - r * np.sin(t), h], axis=1)
    d = rng.normal(size=(N_SPHERE, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sphere = np.array([-0.45, 0.5, 1.8]) + (0.35 + noise(N_SPHERE))[:, None] * d
    local = np.concatenate([wall, pier, vault, sphere])
    return (p0 + local @ R0.T).astype(np.float32)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import synth

    d = tmp_path_factory.mktemp("cylinders_cli")
    poses, ts = synth.make_trajectory(4, spacing=0.12)
    pts = scene_points(poses[0, :3], npo.quat_to_rot(*poses[0, 3:7]))
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
    read = np.loadtxt(d / "odo.txt", dtype=np.float64, ndmin=2)
    return dict(dir=d, pts=pts, poses=read[:, 1:8], ts=read[:, 0])


def _library(ds, cylinders):
    """the facets and the per-facet maps of the command line's colour result through the pipeline"""
    from pointcloudprocessor_amd import capi, pipeline, synth

    eng = pipeline.HipEngine(0)
    try:
        cam = capi.default_camera()
        cam.image_width, cam.image_height = W, H
        eng.configure(cam, capi.default_cull_params())
        pts = ds["pts"]
        eng.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
        eng.ctx.set_frames(ds["poses"])
        eng.ctx.set_image_adjust(True)
        for k in range(len(ds["poses"])):
            eng.ctx.upload_image(k, synth.make_image(k, W, H))
        col = pipeline.PointCloudColorizer(eng)
        col.run(download=False)
        viewer = ds["poses"][:, :3].mean(axis=0)
        before = eng.ctx.download_result_packed().copy()
        fac = col.facets(xyz=pts, normal_radius=0.1, cylinders=cylinders, cylinder_gsd=GSD, viewer=viewer, **FACET)
        maps = col.ortho_maps_by_facet(GSD, xyz=pts, fill_radius=2, viewer=viewer, cylinders=cylinders)
        assert np.array_equal(eng.ctx.download_result_packed(), before), "the colour result is left alone"
        return fac, maps
    finally:
        eng.close()


def _g(v):
    return float("%.9g" % v)


def test_kinds_directories_and_files(dataset, tmp_path):
    from pointcloudprocessor_amd import capi

    ds = dataset
    common = ("--skip_filtered_dumps", "1", "--facets", "1", "--orthoMap", "1", "--orthoFrame", "facets", "--orthoGsd", str(GSD), "--orthoFill", "2")
    plain = geometry_cli._cli(ds, tmp_path / "plain", *common)
    assert plain.returncode == 0, plain.stderr[-2000:]
    off = geometry_cli._cli(ds, tmp_path / "off", *common, "--facetCylinders", "0")
    assert off.returncode == 0, off.stderr[-2000:]
    run = geometry_cli._cli(ds, tmp_path / "run", *common, "--facetCylinders", "1")
    assert run.returncode == 0, run.stderr[-2000:]
    a, b, c = (geometry_cli._files(tmp_path / k) for k in ("plain", "off", "run"))
    assert a == b, "without the flag every file is what it was"
    fac, maps = _library(ds, True)
    old_fac, old_maps = _library(ds, False)
    assert "kind" not in old_fac and "cylinder" not in old_fac and all("kind" not in m for m in old_maps)
    # the four structures: the facet of each by its first point's label
    first = np.cumsum([0, N_WALL, N_PIER, N_VAULT])
    rows = [int(np.flatnonzero(fac["ids"] == fac["label"][i])[0]) for i in first]
    kinds = [int(fac["kind"][r]) for r in rows]
    print("facets", fac["facets"], "kinds", fac["kind"], "of wall / pier / vault / sphere", kinds,
          "cylinder rms", [None if cy is None else cy["stats"]["rms"] for cy in fac["cylinder"]])
    assert len(set(rows)) == 4 and kinds == [1, 2, 2, 0]
    pier, vault, ball = (fac["cylinder"][r] for r in rows[1:])
    assert abs(pier["frame"]["radius"] - 0.4) < 2e-3 and pier["frame"]["side"] == -1 and pier["stats"]["arc"] > 6.2
    assert abs(vault["frame"]["radius"] - 1.0) < 5e-3 and vault["frame"]["side"] == 1 and abs(vault["stats"]["arc"] - np.pi) < 0.05
    assert ball is None or ball["stats"]["rms"] > 0.01
    # one directory per planar and per cylindrical facet, none for the sphere; the planar ones are what they were
    assert sorted(m["row"] for m in maps) == sorted(rows[:3]) and [m["row"] for m in old_maps] == [rows[0]]
    new = [f"ortho/facet_{r}/{name}" for r in rows[1:3] for name in ORTHO]
    assert sorted(c) == sorted(list(a) + new)
    assert all(c[k] == a[k] for k in a if k != "facets/facets.json"), "every other output file is byte for byte the same"
    # facets.json: the old records plus kind and cylinder
    was, now = json.loads(a["facets/facets.json"]), json.loads(c["facets/facets.json"])
    assert len(was) == len(now) == fac["facets"]
    for r, (old, rec) in enumerate(zip(was, now)):
        cy = fac["cylinder"][r]
        assert {k: v for k, v in rec.items() if k not in ("kind", "cylinder")} == old
        assert rec["kind"] == int(fac["kind"][r]) and ("cylinder" in rec) == (cy is not None)
        if cy is not None:
            got = rec["cylinder"]
            assert capi.cyl_frame({k: got[k] for k in CYL_KEYS}).as_dict() == cy["frame"]
            assert got["rows"] == cy["stats"]["rows"] and got["rms"] == _g(cy["stats"]["rms"]) and got["arc"] == _g(cy["stats"]["arc"])
            assert got["eigenvalues"] == [_g(cy["stats"][k]) for k in ("ev0", "ev1", "ev2")]
    # the layers of every directory are the pipeline's, under the frame in ortho_frame.json
    for m in maps:
        d = tmp_path / "run" / "ortho" / f"facet_{m['row']}"
        meta = json.loads((d / "ortho_frame.json").read_text())
        if m["kind"] == 2:
            assert meta["kind"] == "cylinder" and capi.cyl_frame({k: meta[k] for k in CYL_KEYS}).as_dict() == m["frame"]
        else:
            assert "kind" not in meta
            assert capi.ortho_frame({k: meta[k] for k in ("o", "u", "v", "n", "gsd", "width", "height", "d_min", "d_max")}).as_dict() == m["frame"]
        for name, key, descr in LAYERS:
            got = np.load(d / f"{name}.npy")
            assert got.dtype == np.dtype(descr) and got.shape == m[key].shape and got.tobytes() == m[key].tobytes(), (m["row"], name)
        assert (meta["fill_radius"], meta["contributors"], meta["occupied"], meta["filled"]) == (2, m["contributors"], m["occupied"], m["filled"])
        index = m["index"][m["status"] == 1]
        print("facet row", m["row"], "kind", m["kind"], m["index"].shape, "occupied", m["occupied"], "filled", m["filled"])
        # (the command line's camera is the 4096 x 3000 sensor's, and a 1024 x 750 test image is its upper left corner, 12 x 9
        # degrees: few rows of a facet carry a colour, and only those are drawn.  The frames above are compared whole, which is
        # where a wrong viewer or sign would show; the densely coloured maps, the marks and the stripe are
        # test_pipeline_cylinders_gpu.py's, the maps of thousands of rows against the host twin test_ortho_cyl_gpu.py's)
        assert len(index) >= 1 and m["contributors"] >= m["occupied"] == len(index)
        assert (fac["label"][index] == m["facet"]).all(), "only the facet's own points are drawn"
        if m["kind"] == 2:  # the depth layer is the radial deviation: millimetres on these cylinders
            assert np.abs(m["depth"][m["status"] == 1]).max() < 0.01
    assert "2 cylindrical facets of" in run.stdout


def test_texture_skips_the_cylindrical_facets_by_name(dataset, tmp_path):
    ds = dataset
    run = geometry_cli._cli(ds, tmp_path / "run", "--skip_filtered_dumps", "1", "--facets", "1", "--facetCylinders", "1", "--orthoMap", "1",
                            "--orthoFrame", "facets", "--orthoGsd", "0.05", "--orthoTexture", "2")
    assert run.returncode == 0, run.stderr[-2000:]
    files = geometry_cli._files(tmp_path / "run")
    rows = json.loads(files["facets/facets.json"])
    for r, rec in enumerate(rows):
        photo = any(k.startswith(f"ortho/facet_{r}/ortho_photo") for k in files)
        assert photo == (rec["kind"] == 1)
        if rec["kind"] == 2:
            assert f"facet {rec['id']} (ortho/facet_{r}/): cylindrical, skipped by --orthoTexture" in run.stderr
            assert f"ortho/facet_{r}/ortho_rgb.npy" in files
    assert sum(rec["kind"] == 2 for rec in rows) == 2


@pytest.mark.parametrize("flags, needles", [
    (("--facetCylinders", "1"), ("--facetCylinders 1", "--facets 1")),
    (("--facetCylinders", "1", "--facets", "0"), ("--facetCylinders 1", "--facets 1")),
    (("--facetCylinders", "1", "--facets", "1", "--gpus", "2"), ("--facets 1", "--gpus", "index shard")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, needles):
    p = geometry_cli._cli(dataset, tmp_path / "out", *flags)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"


def test_pipeline_refuses_index_shards_and_facets_without_cylinders():
    from pointcloudprocessor_amd import pipeline

    for call in (lambda p: p.facets(cylinders=True), lambda p: p.ortho_maps_by_facet(0.01, cylinders=True)):
        with pytest.raises(ValueError) as e:
            call(pipeline.PointCloudColorizer(None, rank=0, world=2))
        assert "index shard" in str(e.value)
