"""Orthophotos of unrolled maps through the pipeline and the command line ("Orthophotos of unrolled maps", CT6).

Pipeline: test_pipeline_cylinders_gpu.py's scene (a vault of R 3 seen from inside, a closed pier of R 0.3 seen from outside, a
stripe of known width painted on the vault through the keyframes' crack masks) with ortho_maps_by_facet(texture=, cylinders=True,
texture_cylinders=True): each cylindrical map's photo is a direct ortho_texture_cyl's, and the stripe is met on the photo's mask
layer at the arc position where ortho_crack_layers puts it on the map, within that file's bound: two pixel footprints at the
farthest credited range over the smallest incidence cosine.

Command line: test_cli_cylinders_gpu.py's dataset (a wall, a pier, a vault, a sphere).  --orthoTextureCylinders 1 writes the photo
files of every cylindrical facet, byte for byte the pipeline's; without the flag (or with 0) the files are the parent flags'; the
refusals name the flags."""
import json

import numpy as np
import pytest

import _crack_fuse_ref as cf_ref
import _crack_width_ref as cw_ref
import _ortho_cyl_ref as cyl
import test_cli_cylinders_gpu as cyl_cli
import test_cli_geometry_gpu as geometry_cli
import test_pipeline_cylinders_gpu as scene
from test_cli_cylinders_gpu import dataset  # noqa: F401  (the fixture)
from test_crack_fuse_gpu import _inputs

pytestmark = pytest.mark.gpu

GSD, SCALE = 0.01, 2
TEXTURE = dict(scale=SCALE, views=1, interpolate=True, max_step=0.05)
PHOTO = (("ortho_photo_rgb", "rgb", "|u1"), ("ortho_photo_mask", "mask", "|u1"), ("ortho_photo_view", "view", "<i2"),
         ("ortho_photo_status", "status", "|u1"))
PHOTO_FILES = [name + ".npy" for name, _, _ in PHOTO] + ["ortho_photo.json"]
LAYERS = ("rgb", "mask", "status", "view", "count")
COUNTS = ("surface", "textured", "unseen", "skipped_pairs")
_STATE = {}


def _run():
    """the scene through the pipeline, once: colours, the crack chain, the facets with their cylinders, the unrolled maps with
    their photos, and a direct ortho_texture_cyl of each cylindrical map"""
    if _STATE:
        return _STATE
    from pointcloudprocessor_amd import capi, pipeline, synth

    cam = cw_ref.camera(scene.SHAPE)
    poses = cf_ref.stripe_scene()["poses"]
    pts = scene.scene_points()
    c2w = [capi.pose_to_matrices(p)[1] for p in poses]
    masks = [scene.stripe_mask(cam, m) for m in c2w]
    h, w = scene.SHAPE
    eng = pipeline.HipEngine(0)
    try:
        eng.configure(cam, capi.default_cull_params())
        eng.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
        eng.set_keyframes(poses, images=[synth.make_image(k, w, h) for k in range(len(poses))], masks=masks)
        col = pipeline.PointCloudColorizer(eng)
        col.run(download=False)
        cracks = col.crack_map()
        inputs = _inputs(eng.ctx, range(len(poses)), 0, 150)
        fac = col.facets(xyz=pts, normal_radius=0.05, cylinders=True, cylinder_gsd=GSD, **scene.FACET)
        packed = eng.ctx.download_result_packed().copy()
        maps = col.ortho_maps_by_facet(GSD, xyz=pts, texture=TEXTURE, cylinders=True, texture_cylinders=True)
        plain = col.ortho_maps_by_facet(GSD, xyz=pts, texture=TEXTURE, cylinders=True)
        direct = {}
        for m in maps:
            if m["kind"] != 2:
                continue
            eng.ctx.ortho_begin_cyl(m["frame"])
            try:
                eng.ctx.ortho_add_facet(m["facet"], 0)
                eng.ctx.ortho_finish(0)
                direct[m["row"]] = eng.ctx.ortho_texture_cyl(**TEXTURE)
            finally:
                eng.ctx.ortho_end()
        assert np.array_equal(eng.ctx.download_result_packed(), packed), "the colour result is left alone"
        for m in maps:
            m.update(pipeline.ortho_crack_layers(m["index"], cracks["width_mean"], cracks["label"]))
    finally:
        eng.close()
    _STATE.update(cam=cam, poses=poses, pts=pts, c2w=c2w, cracks=cracks, inputs=inputs, fac=fac, maps=maps, plain=plain, direct=direct)
    return _STATE


def test_the_cylindrical_maps_photo_is_a_direct_calls_and_the_default_is_unchanged():
    s = _run()
    kinds = [m["kind"] for m in s["maps"]]
    assert kinds.count(2) == 2 and len(s["direct"]) == 2, kinds
    for m, p in zip(s["maps"], s["plain"]):
        assert m["row"] == p["row"] and m["kind"] == p["kind"]
        assert ("photo" in p) == (p["kind"] == 1), "without the keyword the cylindrical maps carry no photo, as before"
        for key in ("index", "depth", "rgb", "status", "source"):
            assert m[key].tobytes() == p[key].tobytes(), key
        if m["kind"] == 1:
            assert all(m["photo"][k].tobytes() == p["photo"][k].tobytes() for k in LAYERS)
            continue
        photo, want = m["photo"], s["direct"][m["row"]]
        fr = m["frame"]
        assert photo["rgb"].shape == (SCALE * fr["height"], SCALE * fr["width"], 3)
        for key in LAYERS:
            assert photo[key].tobytes() == want[key].tobytes(), (m["row"], key)
        for key in COUNTS:
            assert photo[key] == want[key], (m["row"], key)
        print("facet row", m["row"], "side", fr["side"], photo["rgb"].shape, {k: photo[k] for k in COUNTS})
        assert photo["textured"] >= 0.3 * photo["surface"] > 0 and len(np.unique(photo["view"])) >= 3


def test_the_stripe_is_met_on_the_photos_mask_layer_where_the_crack_layers_put_it():
    s = _run()
    fac = s["fac"]
    row = int(np.flatnonzero(fac["ids"] == fac["label"][0])[0])
    m = next(x for x in s["maps"] if x["row"] == row)
    assert m["kind"] == 2 and m["frame"]["side"] == 1
    cracks, pts = s["cracks"], s["pts"].astype(np.float64)
    # the bound of test_pipeline_cylinders_gpu.py::test_a_stripe_of_known_width_on_the_vault
    far, cos_min = 0.0, 1.0
    for f, (index, pixel, rng, flags, _) in s["inputs"].items():
        ok = (flags.ravel()[pixel] & cf_ref.WIDTH) != 0
        assert ok.any(), f
        p = pts[index[ok]]
        eye = np.asarray(s["c2w"][f], np.float64).reshape(3, 4)[:, 3]
        normal = np.stack([p[:, 0], np.zeros(len(p)), p[:, 2]], axis=1) / np.hypot(p[:, 0], p[:, 2])[:, None]
        v = p - eye
        far = max(far, float(rng[ok].max()))
        cos_min = min(cos_min, float((np.abs((v * normal).sum(axis=1)) / np.linalg.norm(v, axis=1)).min()))
    bound = 2.0 * (far / s["cam"]["fx"]) / cos_min
    fr, photo = m["frame"], m["photo"]
    fine = fr["gsd"] / SCALE
    # where ortho_crack_layers puts the stripe: the columns of the map's pixels whose point belongs to a crack that was seen
    drawn = m["status"] == 1
    at = np.where(drawn, m["index"], 0).astype(np.int64)
    pick = drawn & (m["crack"] >= 0) & (cracks["views"][at] > 0)
    # (the keyframe at the identity sees +-(H / 2) / fy of the range up and down the vault; the band is W0 wide: half of that
    # rectangle's pixels is the floor, on the map and on the photo)
    seen = 2.0 * (scene.SHAPE[0] / 2.0 / s["cam"]["fy"]) * scene.R_VAULT
    assert pick.sum() >= 0.5 * (scene.W0 / fr["gsd"]) * (seen / fr["gsd"])
    layer_arc = (np.nonzero(pick)[1] + 0.5) * fr["gsd"]
    rows, cols = np.nonzero(photo["mask"] > 0)
    photo_arc = (cols + 0.5) * fine
    centre = np.array([[scene.R_VAULT * np.sin(scene.ARC0 / scene.R_VAULT), 0.0, scene.R_VAULT * np.cos(scene.ARC0 / scene.R_VAULT)]], np.float32)
    _, x, _, _ = cyl.coords(fr, centre)
    painted = float(x[0]) * fr["gsd"]
    print(f"stripe on the photo: {len(cols)} mask pixels, arc {photo_arc.min():.4f} .. {photo_arc.max():.4f} m, mean {photo_arc.mean():.4f}; the "
          f"crack layer's pixels {layer_arc.min():.4f} .. {layer_arc.max():.4f} m, mean {layer_arc.mean():.4f}; painted centre {painted:.4f} m, "
          f"width {scene.W0} m; bound {bound * 1e3:.3f} mm (farthest range {far:.3f} m, cos_min {cos_min:.4f})")
    assert len(cols) >= 0.5 * (scene.W0 / fine) * (seen / fine)
    # (a mask pixel of the photo is a texel of the painted band up to the mask's edge placement, its centre within half a fine pixel)
    assert np.abs(photo_arc - painted).max() <= scene.W0 / 2 + bound + 0.5 * fine
    # against the map's own crack layer: the same band, so the two spans agree within the bound and a map pixel
    assert abs(photo_arc.mean() - layer_arc.mean()) <= bound
    assert layer_arc.min() - bound - fr["gsd"] <= photo_arc.min() and photo_arc.max() <= layer_arc.max() + bound + fr["gsd"]
    assert photo_arc.max() - photo_arc.min() >= scene.W0 - 2 * bound, "the band keeps its width on the photo"
    assert rows.max() - rows.min() > 0.9 * seen / fine, "the stripe runs as far along the vault as the keyframes see it"


def _library(ds, texture_cylinders):
    """test_cli_cylinders_gpu._library with the photos: the per-facet maps of the command line's colour result"""
    from pointcloudprocessor_amd import capi, pipeline, synth

    W, H = cyl_cli.W, cyl_cli.H
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
        col.facets(xyz=pts, normal_radius=0.1, cylinders=True, cylinder_gsd=0.05, viewer=viewer, **cyl_cli.FACET)
        return col.ortho_maps_by_facet(0.05, xyz=pts, viewer=viewer, texture=dict(scale=2), cylinders=True, texture_cylinders=texture_cylinders)
    finally:
        eng.close()


def test_the_command_line_writes_the_pipelines_photos_and_is_unchanged_without_the_flag(dataset, tmp_path):  # noqa: F811
    ds = dataset
    parent = ("--skip_filtered_dumps", "1", "--facets", "1", "--facetCylinders", "1", "--orthoMap", "1", "--orthoFrame", "facets", "--orthoGsd",
              "0.05", "--orthoTexture", "2")
    was = geometry_cli._cli(ds, tmp_path / "was", *parent)
    off = geometry_cli._cli(ds, tmp_path / "off", *parent, "--orthoTextureCylinders", "0")
    run = geometry_cli._cli(ds, tmp_path / "run", *parent, "--orthoTextureCylinders", "1")
    for p in (was, off, run):
        assert p.returncode == 0, p.stderr[-2000:]
    a, b, c = (geometry_cli._files(tmp_path / k) for k in ("was", "off", "run"))
    assert a == b, "with 0 every file is what the parent's flags write"
    skipped = [ln for ln in was.stderr.splitlines() if "cylindrical, skipped by --orthoTexture" in ln]
    assert len(skipped) == 2 and skipped == [ln for ln in off.stderr.splitlines() if "skipped by --orthoTexture" in ln]
    assert "skipped" not in run.stderr
    rows = json.loads(c["facets/facets.json"])
    cyl_rows = [r for r, rec in enumerate(rows) if rec["kind"] == 2]
    assert len(cyl_rows) == 2
    new = [f"ortho/facet_{r}/{name}" for r in cyl_rows for name in PHOTO_FILES]
    assert sorted(c) == sorted(list(a) + new)
    assert all(c[k] == a[k] for k in a), "every other output file is byte for byte the same"
    maps = _library(ds, True)
    plain = _library(ds, False)
    assert [m["row"] for m in maps] == [m["row"] for m in plain]
    for m, p in zip(maps, plain):
        d = tmp_path / "run" / "ortho" / f"facet_{m['row']}"
        assert ("photo" in p) == (m["kind"] == 1) and "photo" in m
        if m["kind"] == 1:  # the planar facets' photos do not change with the keyword
            assert all(m["photo"][k].tobytes() == p["photo"][k].tobytes() for k in LAYERS)
        for name, key, descr in PHOTO:
            got = np.load(d / f"{name}.npy")
            want = m["photo"][key]
            assert got.dtype == np.dtype(descr) and got.shape == want.shape and got.tobytes() == want.tobytes(), (m["row"], name)
        info = json.loads((d / "ortho_photo.json").read_text())
        fr = m["frame"]
        assert (info["scale"], info["views"], info["interpolate"], info["width"], info["height"], info["calls"]) == \
               (2, 1, 1, 2 * fr["width"], 2 * fr["height"], 1)
        assert (info["surface"], info["textured"], info["unseen"], info["skipped_pairs"]) == \
               tuple(m["photo"][k] for k in ("surface", "textured", "unseen", "skipped_pairs"))
        print("facet row", m["row"], "kind", m["kind"], m["photo"]["rgb"].shape, {k: info[k] for k in ("surface", "textured", "unseen")})
        assert info["surface"] >= 1


@pytest.mark.parametrize("flags", [
    ("--orthoTextureCylinders", "1"),
    ("--orthoTextureCylinders", "1", "--facets", "1", "--facetCylinders", "1", "--orthoMap", "1", "--orthoFrame", "facets"),
    ("--orthoTextureCylinders", "1", "--facets", "1", "--orthoMap", "1", "--orthoFrame", "facets", "--orthoTexture", "2"),
    ("--orthoTextureCylinders", "1", "--facets", "1", "--facetCylinders", "1", "--orthoMap", "1", "--orthoTexture", "2"),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags):  # noqa: F811
    p = geometry_cli._cli(dataset, tmp_path / "out", *flags)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in ("--orthoTextureCylinders 1", "--orthoTexture k", "--facetCylinders 1", "--orthoFrame facets"):
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
