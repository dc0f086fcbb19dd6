"""--orthoTexture k / --orthoTextureViews m / --orthoTextureInterp 0|1 / --orthoTextureStep s end to end (DESIGN.md,
"Orthophotos"): the five files of the command line hold, bit for bit, what capi returns for the frame in ortho_frame.json on the
same colour result; the other ortho files and every other output are byte for byte those of a run without the flag;
--enableMLS 1 --streamColour 1 writes the files of the same run without --streamColour; the refusals name the flag."""
import json

import numpy as np
import pytest

import test_cli_geometry_gpu as geometry_cli
import test_cli_stream_colour_gpu as stream_cli
from test_cli_geometry_gpu import dataset as geometry_dataset  # noqa: F401  (a curved wall, four keyframes, stray and far points)
from test_cli_stream_colour_gpu import dataset as stream_dataset  # noqa: F401  (the wall in view of six keyframes, with masks)

pytestmark = pytest.mark.gpu

W, H = 1024, 750
PHOTO = (("ortho_photo_rgb", "rgb", "|u1"), ("ortho_photo_mask", "mask", "|u1"), ("ortho_photo_view", "view", "<i2"),
         ("ortho_photo_status", "status", "|u1"))
NEW = ["ortho/ortho_photo_rgb.npy", "ortho/ortho_photo_mask.npy", "ortho/ortho_photo_view.npy", "ortho/ortho_photo_status.npy",
       "ortho/ortho_photo.json"]


def _library(ds, frame, fill, texture):
    """the map and the photo of the command line's colour result through capi: default camera and cull, adjusted images"""
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
        return col.ortho_map(frame, fill_radius=fill, texture=texture)
    finally:
        eng.close()


def test_the_five_files_hold_the_librarys_photo_and_nothing_else_changes(geometry_dataset, tmp_path):  # noqa: F811
    ds = geometry_dataset
    common = ("--skip_filtered_dumps", "1", "--orthoMap", "1", "--orthoGsd", "0.02", "--orthoFill", "2")
    plain = geometry_cli._cli(ds, tmp_path / "plain", *common)
    assert plain.returncode == 0, plain.stderr[-2000:]
    photo = geometry_cli._cli(ds, tmp_path / "photo", *common, "--orthoTexture", "3", "--orthoTextureViews", "5", "--orthoTextureInterp", "1",
                              "--orthoTextureStep", "0.03")
    assert photo.returncode == 0, photo.stderr[-2000:]
    a, c = geometry_cli._files(tmp_path / "plain"), geometry_cli._files(tmp_path / "photo")
    assert not any("photo" in k for k in a)
    assert sorted(c) == sorted(list(a) + NEW) and all(c[k] == a[k] for k in a), "every other output file is byte for byte the same"
    meta = json.loads((tmp_path / "photo" / "ortho" / "ortho_frame.json").read_text())
    frame = {k: meta[k] for k in ("o", "u", "v", "n", "gsd", "width", "height", "d_min", "d_max")}
    want = _library(ds, frame, 2, dict(scale=3, views=5, interpolate=True, max_step=0.03))["photo"]
    h, w = frame["height"] * 3, frame["width"] * 3
    for name, key, descr in PHOTO:
        got = np.load(tmp_path / "photo" / "ortho" / f"{name}.npy")
        assert got.dtype == np.dtype(descr) and got.shape == want[key].shape and got.shape[:2] == (h, w), name
        assert got.tobytes() == want[key].tobytes(), name
    info = json.loads((tmp_path / "photo" / "ortho" / "ortho_photo.json").read_text())
    assert (info["scale"], info["views"], info["interpolate"], info["width"], info["height"], info["calls"]) == (3, 5, 1, w, h, 1)
    assert np.float32(info["max_step"]) == np.float32(0.03) and np.float32(info["gsd"]) == np.float32(frame["gsd"]) / np.float32(3)
    assert (info["surface"], info["textured"], info["unseen"], info["skipped_pairs"]) == (want["surface"], want["textured"], want["unseen"],
                                                                                         want["skipped_pairs"])
    assert want["textured"] > 1000 and f"{want['textured']} textured" in photo.stdout
    assert not want["mask"].any(), "the run has no masks"
    # the defaults: the sharpest view, interpolated across 0.05 m
    dflt = geometry_cli._cli(ds, tmp_path / "dflt", *common, "--orthoTexture", "2")
    assert dflt.returncode == 0, dflt.stderr[-2000:]
    want2 = _library(ds, frame, 2, dict(scale=2))["photo"]
    for name, key, _ in PHOTO:
        assert np.load(tmp_path / "dflt" / "ortho" / f"{name}.npy").tobytes() == want2[key].tobytes(), name


def test_streamed_files_are_the_one_shot_files(stream_dataset, tmp_path):  # noqa: F811
    common = ("--fuseMasks", "1", "--skip_filtered_dumps", "1", "--orthoMap", "1", "--orthoGsd", "0.01", "--orthoFill", "1", "--orthoTexture", "2",
              "--orthoTextureViews", "5")
    one = stream_cli._cli(stream_dataset, tmp_path / "one", *common, "--streamColour", "0")
    assert one.returncode == 0, one.stderr[-2000:]
    st = stream_cli._cli(stream_dataset, tmp_path / "streamed", *common, "--streamColour", "1", "--streamChunk", "4096")
    assert st.returncode == 0, st.stderr[-2000:]
    for name in [k.split("/")[1] for k in NEW] + ["ortho_rgb.npy", "ortho_index.npy", "ortho_frame.json"]:
        a, b = (tmp_path / "one" / "ortho" / name).read_bytes(), (tmp_path / "streamed" / "ortho" / name).read_bytes()
        assert a == b, name
    info = json.loads((tmp_path / "streamed" / "ortho" / "ortho_photo.json").read_text())
    mask = np.load(tmp_path / "streamed" / "ortho" / "ortho_photo_mask.npy")
    view = np.load(tmp_path / "streamed" / "ortho" / "ortho_photo_view.npy")
    assert info["textured"] > 4000 and len(np.unique(view)) >= 3 and 0 < (mask == 255).sum() < info["textured"], "masks reach the photo"


@pytest.mark.parametrize("flags, needles", [
    (("--orthoTexture", "4"), ("--orthoTexture", "--orthoMap 1")),
    (("--orthoMap", "1", "--orthoTexture", "4", "--gpus", "2"), ("--orthoTexture", "--gpus", "index shard")),
    (("--orthoMap", "1", "--orthoTexture", "4", "--cull", "hpr"), ("--orthoTexture", "--cull hpr", "depth maps")),
    (("--orthoMap", "1", "--orthoTexture", "17"), ("--orthoTexture", "invalid")),
    (("--orthoMap", "1", "--orthoTexture", "4", "--orthoTextureViews", "6"), ("--orthoTextureViews", "invalid")),
    (("--orthoMap", "1", "--orthoTexture", "4", "--orthoTextureStep", "0"), ("--orthoTextureStep", "invalid")),
    (("--orthoMap", "1", "--orthoTextureViews", "5"), ("--orthoTextureViews", "--orthoTexture k")),
])
def test_refusals_name_the_flags(geometry_dataset, tmp_path, flags, needles):  # noqa: F811
    p = geometry_cli._cli(geometry_dataset, tmp_path / "out", *flags)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
