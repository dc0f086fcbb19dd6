"""--crackDirection 1 / --crackUp end to end ("Crack directions on the map"): the two .npy files of the command line
hold, bit for bit, what capi's crack_directions returns for the same map, poses and mask files, and crack_directions_3d.json
what crack_axis_host makes of the fetched rows (its floats as "%.9g" prints them); every other file is byte for byte that of a
run without the flag; three painted stripes come out vertical, horizontal and diagonal; on a pier a ring crack and a generator
crack come out circumferential and longitudinal; the refusals name the flags."""
import json

import numpy as np
import pytest

from test_cli_crack_width_gpu import _cli, _files, dataset  # noqa: F401  (the wall patch, three keyframes, crack masks)

pytestmark = pytest.mark.gpu

W, H = 1024, 750
NEW = ["crack_width/map_tangent.npy", "crack_width/map_anisotropy.npy", "crack_width/crack_directions_3d.json"]


def _g(v):
    return float("%.9g" % v)


def _context(pts, poses, masks):
    from pointcloudprocessor_amd import capi

    ctx = capi.Context(0)
    cam = capi.default_camera()
    cam.image_width, cam.image_height = W, H
    ctx.set_camera(cam, capi.default_cull_params())
    ctx.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
    ctx.set_frames(poses)
    for k, m in enumerate(masks):
        ctx.upload_mask(k, m)
    return ctx


def _library(ds, threshold, radius, min_views, link):
    ctx = _context(ds["pts"], ds["poses"], ds["masks"])
    try:
        ctx.crack_fuse_begin()
        for k in range(len(ds["masks"])):
            ctx.crack_fuse_add(k, threshold, radius)
        out = ctx.crack_directions(min_views, link)
        ctx.crack_fuse_end()
        return out
    finally:
        ctx.close()


def _klass(axis, up):
    if not np.any(axis):
        return 0.0, "none"
    incl = float(np.degrees(np.arccos(min(1.0, abs(float(np.dot(axis, up)))))))
    return incl, "vertical" if incl < 22.5 else "horizontal" if incl > 67.5 else "diagonal"


def test_files_hold_the_librarys_arrays_and_nothing_else_changes(dataset, tmp_path):  # noqa: F811
    up = np.array([1.0, -2.0, 2.0]) / 3.0
    fused = _cli(dataset, tmp_path / "fused", "--crackFuse", "1", "--crackLength", "1", "--crackLinkRadius", "0.05")
    assert fused.returncode == 0, fused.stderr[-2000:]
    both = _cli(dataset, tmp_path / "both", "--crackFuse", "1", "--crackLength", "1", "--crackDirection", "1", "--crackUp", "2,-4,4",
                "--crackLinkRadius", "0.05", timing=tmp_path / "phases.json")
    assert both.returncode == 0, both.stderr[-2000:]
    a, c = _files(tmp_path / "fused"), _files(tmp_path / "both")
    assert "crack_width/cracks_3d.json" in a and "crack_width/crack_lengths_3d.json" in a and not any(k in a for k in NEW)
    assert sorted(c) == sorted(list(a) + NEW)
    assert all(c[k] == a[k] for k in a), "cracks_3d.json, the lengths and every other output file are byte for byte the same"
    n = len(dataset["pts"])
    want = _library(dataset, 0, 150, 1, 0.05)
    folder = tmp_path / "both" / "crack_width"
    for name, key, shape in (("map_tangent", "tangent", (n, 3)), ("map_anisotropy", "anisotropy", (n,))):
        got = np.load(folder / f"{name}.npy")
        assert got.dtype == np.dtype("<f4") and got.shape == shape and got.tobytes() == want[key].tobytes(), name
    rows = json.loads((folder / "crack_directions_3d.json").read_text())
    assert len(rows) == want["cracks"] >= 1 and [r["id"] for r in rows] == [r["id"] for r in json.loads((folder / "cracks_3d.json").read_text())]
    assert want["axis"].any(axis=1).sum() >= 1 and want["tangent"].any(axis=1).sum() > 100, "no crack with an axis: the scene is wrong"
    for row, cid, links, axis, an in zip(rows, want["ids"], want["link_count"], want["axis"], want["axis_anisotropy"]):
        assert set(row) == {"id", "links", "axis", "anisotropy", "inclination_deg", "class"}
        assert (row["id"], row["links"]) == (int(cid), int(links))
        assert row["axis"] == [_g(v) for v in axis] and row["anisotropy"] == _g(an)
        incl, cls = _klass(axis, up)
        assert abs(row["inclination_deg"] - incl) <= 1e-6 and 0.0 <= row["inclination_deg"] <= 90.0
        if min(abs(incl - 22.5), abs(incl - 67.5)) > 1e-6:
            assert row["class"] == cls
    assert f"{want['cracks']} cracks" in both.stdout
    phases = json.loads((tmp_path / "phases.json").read_text())  # the binary's own split
    assert phases["crack_direction_gpu_s"] > 0 and phases["crack_direction_write_s"] > 0 and phases["crack_fuse_gpu_s"] > 0


def _write_dataset(d, pts, poses, ts, masks):
    from pointcloudprocessor_amd import synth

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
            with open(d / ("%f.pgm" % t), "wb") as g:
                g.write(b"P5\n%d %d\n255\n" % (W, H) + masks[k].tobytes())
    read = np.loadtxt(d / "odo.txt", dtype=np.float64, ndmin=2)
    return dict(dir=d, pts=pts, poses=read[:, 1:8], ts=read[:, 0], masks=masks)


def _first_axes():
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import synth

    poses, ts = synth.make_trajectory(1, spacing=0.12)
    return poses, ts, poses[0, :3], npo.quat_to_rot(*poses[0, 3:7])  # (the columns: right, down, forward in the world)


def _stripe(mask, x0, y0, x1, y1, half):
    """a straight stripe from pixel (x0, y0) to (x1, y1), `half` pixels to either side"""
    yy, xx = np.mgrid[0:H, 0:W]
    dx, dy = x1 - x0, y1 - y0
    t = np.clip(((xx - x0) * dx + (yy - y0) * dy) / float(dx * dx + dy * dy), 0.0, 1.0)
    mask[np.hypot(xx - (x0 + t * dx), yy - (y0 + t * dy)) <= half] = 255


def test_stripes_come_out_vertical_horizontal_and_diagonal(tmp_path):
    """one keyframe before a slanted wall (depth 1.9 + 0.2 a along the camera's right axis a) with three straight stripes in its
    mask: down the image, across it, and at 45 degrees.  With the camera's down axis as --crackUp they run at 0, 90 and
    acos(1 / sqrt(2.04)) = 45.6 degrees to it."""
    poses, ts, p0, R0 = _first_axes()
    rng = np.random.default_rng(61)
    n = 300_000  # the 1024 x 750 image is the upper left corner of the sensor: a patch of 0.9 x 0.7 m around what it sees
    a, b = rng.uniform(-0.95, -0.3, n), rng.uniform(-0.7, -0.25, n)
    depth = 1.9 + 0.2 * a + rng.normal(0, 5e-4, n)
    pts = (p0 + a[:, None] * R0[:, 0] + b[:, None] * R0[:, 1] + depth[:, None] * R0[:, 2]).astype(np.float32)
    mask = np.zeros((H, W), np.uint8)
    _stripe(mask, 120, 60, 120, 620, 8)
    _stripe(mask, 330, 700, 990, 700, 8)
    _stripe(mask, 470, 50, 870, 450, 8)
    ds = _write_dataset(tmp_path, pts, poses, ts, [mask])
    up = R0[:, 1]
    run = _cli(ds, tmp_path / "run", "--crackFuse", "1", "--crackDirection", "1", "--crackUp", ",".join(repr(float(v)) for v in up))
    assert run.returncode == 0, run.stderr[-2000:]
    rows = json.loads((tmp_path / "run" / "crack_width" / "crack_directions_3d.json").read_text())
    big = sorted(rows, key=lambda r: -r["links"])[:3]
    print([(r["id"], r["links"], r["class"], r["inclination_deg"], r["anisotropy"]) for r in sorted(rows, key=lambda r: -r["links"])[:6]])
    assert len(rows) >= 3 and big[2]["links"] > 10 * (sorted(rows, key=lambda r: -r["links"])[3]["links"] if len(rows) > 3 else 0), \
        "the three stripes are not the three large cracks: the scene is wrong"
    got = {r["class"]: r for r in big}
    assert set(got) == {"vertical", "horizontal", "diagonal"}
    assert got["vertical"]["inclination_deg"] < 3.0 and got["horizontal"]["inclination_deg"] > 87.0
    assert abs(got["diagonal"]["inclination_deg"] - np.degrees(np.arccos(1.0 / np.sqrt(2.04)))) < 3.0
    assert all(r["anisotropy"] > 0.9 for r in big)
    tangent = np.load(tmp_path / "run" / "crack_width" / "map_tangent.npy")
    label = np.load(tmp_path / "run" / "crack_width" / "map_crack.npy")
    mine = (label == got["vertical"]["id"]) & tangent.any(axis=1)
    assert mine.sum() > 100 and np.median(np.degrees(np.arccos(np.minimum(1.0, np.abs(tangent[mine] @ up))))) < 30.0


def test_ring_and_generator_cracks_on_a_pier(tmp_path):
    """a pier of R 0.4 about the camera's down axis where the one keyframe sees it, sampled densely there, with a ring crack and a
    generator crack painted into the mask through the projection of their points: with --facets 1 --facetCylinders 1 they come
    out circumferential and longitudinal on a facet of kind cylinder."""
    from pointcloudprocessor_amd import capi

    poses, ts, p0, R0 = _first_axes()
    rng = np.random.default_rng(62)
    # (right, down, forward); the front of the pier is 1.05 m before the camera: the command line crops the map to 2 m about the
    # keyframes along every world axis, and forward is nearly one of them
    centre = np.array([-0.33, 0.0, 1.45])

    def on_pier(t, h, noise):
        r = 0.4 + noise
        return np.stack([centre[0] + r * np.cos(t), h, centre[2] + r * np.sin(t)], axis=1)

    n_all, n_patch, n_line = 20000, 60000, 3000
    whole = on_pier(rng.uniform(0, 2 * np.pi, n_all), rng.uniform(-0.75, 0.15, n_all), 1e-3 * rng.normal(size=n_all))
    patch = on_pier(np.radians(rng.uniform(250, 290, n_patch)), rng.uniform(-0.34, -0.17, n_patch), 5e-4 * rng.normal(size=n_patch))
    ring = on_pier(np.radians(np.linspace(257, 283, n_line)), np.full(n_line, -0.21), np.zeros(n_line))  # (row ~580, columns 124 .. 942)
    gen = on_pier(np.full(n_line, np.radians(270.0)), np.linspace(-0.328, -0.25, n_line), np.zeros(n_line))  # (column ~518, rows 30 .. 390)
    local = np.concatenate([whole, patch, ring, gen])
    pts = (p0 + local @ R0.T).astype(np.float32)
    first_ring, first_gen = n_all + n_patch, n_all + n_patch + n_line
    # the mask: a disc of 6 pixels about the pixel of every crack-line point
    ctx = _context(pts, poses, [np.zeros((H, W), np.uint8)])
    try:
        pix = ctx.project_frame(0, want_cam=False)["pixel"]
    finally:
        ctx.close()
    seen_ring, seen_gen = pix[first_ring:first_gen] >= 0, pix[first_gen:] >= 0
    print("line points in the image: ring", int(seen_ring.sum()), "generator", int(seen_gen.sum()), "patch", int((pix[n_all:first_ring] >= 0).sum()))
    assert seen_ring.mean() > 0.9 and seen_gen.mean() > 0.9, "the crack lines are not in the image: the scene is wrong"
    mask = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[-6:7, -6:7]
    disc = np.hypot(xx, yy) <= 6
    for p in np.unique(pix[first_ring:][pix[first_ring:] >= 0])[::3].tolist():
        y, x = divmod(p, W)
        y0, y1, x0, x1 = max(y - 6, 0), min(y + 7, H), max(x - 6, 0), min(x + 7, W)
        mask[y0:y1, x0:x1][disc[y0 - y + 6:y1 - y + 6, x0 - x + 6:x1 - x + 6]] = 255
    lo, hi = np.minimum(p0, 1e300) - 2.0, np.maximum(p0, 0.0) + 2.0
    assert ((pts >= lo) & (pts <= hi)).all(), "the crop would drop points and shift the indices: the scene is wrong"
    ds = _write_dataset(tmp_path, pts, poses, ts, [mask])
    run = _cli(ds, tmp_path / "run", "--facets", "1", "--facetCylinders", "1", "--crackFuse", "1", "--crackDirection", "1")
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-2000:]
    folder = tmp_path / "run" / "crack_width"
    rows = {r["id"]: r for r in json.loads((folder / "crack_directions_3d.json").read_text())}
    facets = json.loads((tmp_path / "run" / "facets" / "facets.json").read_text())
    label = np.load(folder / "map_crack.npy")
    ring_ids, gen_ids = label[first_ring:first_gen], label[first_gen:]
    assert (ring_ids >= 0).mean() > 0.5 and (gen_ids >= 0).mean() > 0.5, "the crack lines are not credited: the scene is wrong"
    ring_id = int(np.bincount(ring_ids[ring_ids >= 0]).argmax())
    gen_id = int(np.bincount(gen_ids[gen_ids >= 0]).argmax())
    print("ring", rows[ring_id], "generator", rows[gen_id], "kinds", [f.get("kind") for f in facets])
    assert ring_id != gen_id
    down = R0[:, 1]  # the pier's axis
    for rec, cls in ((rows[ring_id], "circumferential"), (rows[gen_id], "longitudinal")):
        assert rec["facet"] >= 0 and rec["facet_kind"] == "cylinder" and "out_of_plane_deg" not in rec
        fac = next(f for f in facets if f["id"] == rec["facet"])
        assert fac["kind"] == 2 and abs(fac["cylinder"]["radius"] - 0.4) < 5e-3
        want = float(np.degrees(np.arccos(min(1.0, abs(float(np.dot(rec["axis"], fac["cylinder"]["a"])))))))
        assert abs(rec["to_axis_deg"] - want) < 1e-4 and rec["cylinder_class"] == cls
        assert abs(float(np.degrees(np.arccos(min(1.0, abs(float(np.dot(rec["axis"], down))))))) - rec["to_axis_deg"]) < 2.0
    assert rows[ring_id]["to_axis_deg"] > 80.0 and rows[gen_id]["to_axis_deg"] < 10.0
    # against the default --crackUp 0,0,1: the classes are what the inclination says
    for rec in rows.values():
        incl, cls = _klass(np.array(rec["axis"]), np.array([0.0, 0.0, 1.0]))
        assert abs(rec["inclination_deg"] - incl) < 1e-4
        if min(abs(incl - 22.5), abs(incl - 67.5)) > 1e-3:
            assert rec["class"] == cls
    assert capi.PCP_OK == 0


@pytest.mark.parametrize("flags, masks, needles", [
    (("--crackDirection", "1"), True, ("--crackDirection 1", "--crackFuse 1")),
    (("--crackFuse", "1", "--crackDirection", "1", "--crackUp", "0,0,0"), True, ("--crackUp", "invalid", "not zero")),
    (("--crackFuse", "1", "--crackDirection", "1", "--crackUp", "0,1"), True, ("--crackUp", "invalid")),
    (("--crackFuse", "1", "--crackDirection", "1", "--crackUp", "0,nan,1"), True, ("--crackUp", "invalid")),
    (("--crackFuse", "1", "--crackDirection", "1"), False, ("--crackFuse 1", "--mask_image_folder")),
    (("--crackFuse", "1", "--crackDirection", "1", "--gpus", "2"), True, ("--crackFuse 1", "--gpus", "index shard", "not built")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, masks, needles):  # noqa: F811
    p = _cli(dataset, tmp_path / "out", *flags, masks=masks)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"

