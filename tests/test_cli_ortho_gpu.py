"""--orthoMap 1 / --orthoGsd g / --orthoFill R / --orthoFrame end to end ("Orthographic maps"): the .npy files of the
command line hold, bit for bit, what capi returns for the frame in ortho_frame.json on the same colour result; every other
output file is byte for byte the file of a run without the flag; with --crackFuse 1 ortho_width.npy is map_width.npy[index];
--enableMLS 1 --streamColour 1 writes the files of the same run without --streamColour; --gpus 2 is refused by name."""
import json
import re

import numpy as np
import pytest

import test_cli_crack_width_gpu as crack_cli
import test_cli_geometry_gpu as geometry_cli
import test_cli_stream_colour_gpu as stream_cli
from test_cli_crack_width_gpu import dataset as crack_dataset  # noqa: F401  (the wall patch, three keyframes, crack masks)
from test_cli_geometry_gpu import dataset as geometry_dataset  # noqa: F401  (a curved wall, four keyframes, stray and far points)
from test_cli_stream_colour_gpu import dataset as stream_dataset  # noqa: F401  (the wall in view of six keyframes, with masks)

pytestmark = pytest.mark.gpu

W, H = 1024, 750
LAYERS = (("ortho_rgb", "rgb", "|u1"), ("ortho_depth", "depth", "<f4"), ("ortho_index", "index", "<u4"), ("ortho_status", "status", "|u1"))
NEW = ["ortho/ortho_rgb.npy", "ortho/ortho_depth.npy", "ortho/ortho_index.npy", "ortho/ortho_status.npy", "ortho/ortho_frame.json"]


def _library(ds, frame, fill):
    """the map of the command line's colour result through capi: default camera and cull, adjusted images"""
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
        return col.ortho_map(frame, fill_radius=fill)
    finally:
        eng.close()


def _g(v):
    return float("%.9g" % v)


def _check_files(out, ds, fill):
    from pointcloudprocessor_amd import capi

    meta = json.loads((out / "ortho" / "ortho_frame.json").read_text())
    frame = {k: meta[k] for k in ("o", "u", "v", "n", "gsd", "width", "height", "d_min", "d_max")}
    want = _library(ds, frame, fill)
    assert capi.ortho_frame(frame).as_dict() == want["frame"], "the json's numbers are the frame's floats"
    h, w = frame["height"], frame["width"]
    for name, key, descr in LAYERS:
        got = np.load(out / "ortho" / f"{name}.npy")
        assert got.dtype == np.dtype(descr) and got.shape == want[key].shape and got.shape[:2] == (h, w), name
        assert got.tobytes() == want[key].tobytes(), name
    assert (meta["fill_radius"], meta["contributors"], meta["occupied"], meta["filled"]) == (
        fill, want["contributors"], want["occupied"], want["filled"])
    return meta, want


def test_npy_files_hold_the_librarys_layers_and_nothing_else_changes(geometry_dataset, tmp_path):  # noqa: F811
    from pointcloudprocessor_amd import capi

    ds = geometry_dataset
    plain = geometry_cli._cli(ds, tmp_path / "plain", "--skip_filtered_dumps", "1", "--orthoMap", "0", "--orthoGsd", "0.5")
    assert plain.returncode == 0, plain.stderr[-2000:]
    auto = geometry_cli._cli(ds, tmp_path / "auto", "--skip_filtered_dumps", "1", "--orthoMap", "1", "--orthoGsd", "0.02", "--orthoFill", "2")
    assert auto.returncode == 0, auto.stderr[-2000:]
    a, c = geometry_cli._files(tmp_path / "plain"), geometry_cli._files(tmp_path / "auto")
    assert not any(k.startswith("ortho/") for k in a)
    assert sorted(c) == sorted(list(a) + NEW) and all(c[k] == a[k] for k in a), "every other output file is byte for byte the same"
    assert c["ortho/ortho_index.npy"][:8] == b"\x93NUMPY\x01\x00"
    meta, want = _check_files(tmp_path / "auto", ds, 2)
    # (the fifty far points tilt the fitted plane against the wall, which is then seen at a slant: a few hundred pixels)
    assert want["occupied"] > 100 and want["filled"] > 100 and f"{want['occupied']} occupied, {want['filled']} filled" in auto.stdout
    # the auto frame: fitted to the finite points of the map the run read, seen from the mean keyframe position
    fit = capi.ortho_fit_frame_host(ds["pts"], 0.02, has=np.isfinite(ds["pts"]).all(axis=1).astype(np.uint8), viewer=ds["poses"][:, :3].mean(axis=0))
    assert fit.as_dict() == want["frame"]
    assert np.dot(ds["poses"][:, :3].mean(axis=0) - np.array(meta["o"]), np.array(meta["n"])) < 0, "the keyframes look along n"
    # nine numbers: the first keyframe's image axes with the origin past the wall's corner; n = u x v, the window unbounded, the
    # raster sized to the map: every coloured row on the positive side of the origin is drawn -- the wall and the stray points
    # all are, the fifty far points may not be
    from oracle import np_oracle as npo

    R0 = npo.quat_to_rot(*ds["poses"][0, 3:7])  # camera -> world
    o = ds["poses"][0, :3] - 1.2 * R0[:, 0] - 1.2 * R0[:, 1]
    spec = ",".join("%.9g" % x for x in list(o) + list(R0[:, 0]) + list(R0[:, 1]))
    given = geometry_cli._cli(ds, tmp_path / "given", "--skip_filtered_dumps", "1", "--orthoMap", "1", "--orthoGsd", "0.02", "--orthoFrame", spec)
    assert given.returncode == 0, given.stderr[-2000:]
    meta2, want2 = _check_files(tmp_path / "given", ds, 0)
    assert meta2["o"] == [_g(np.float32(_g(x))) for x in o] and meta2["u"] == [_g(np.float32(_g(x))) for x in R0[:, 0]]
    assert np.abs(np.float32(meta2["n"]) - np.float32(R0[:, 2])).max() < 1e-6, "n = u x v"
    assert np.float32(meta2["d_min"]) == -np.finfo(np.float32).max and np.float32(meta2["d_max"]) == np.finfo(np.float32).max
    coloured = int(re.search(rb"^POINTS (\d+)$", a["cloudInWorldWithRGB.pcd"][:400], re.M).group(1))
    print("coloured rows", coloured, "contributors", want2["contributors"], "occupied", want2["occupied"])
    assert coloured > 500 and coloured - 50 <= want2["contributors"] <= coloured
    assert want2["filled"] == 0 and 100 < want2["occupied"] <= want2["contributors"]
    assert (want2["depth"][want2["status"] == 1] > 1.5).sum() > 100, "the wall lies 1.9 m in front of the origin's plane"


def test_crack_layers_are_the_maps_arrays_at_the_index_layer(crack_dataset, tmp_path):  # noqa: F811
    run = crack_cli._cli(crack_dataset, tmp_path / "out", "--skip_filtered_dumps", "1", "--orthoMap", "1", "--orthoGsd", "0.005", "--crackFuse", "1",
                         "--fuseMasks", "1")
    assert run.returncode == 0, run.stderr[-2000:]
    d = tmp_path / "out"
    index = np.load(d / "ortho" / "ortho_index.npy")
    width, crack = np.load(d / "ortho" / "ortho_width.npy"), np.load(d / "ortho" / "ortho_crack.npy")
    label = np.load(d / "ortho" / "ortho_label.npy")
    map_width, map_crack = np.load(d / "crack_width" / "map_width.npy"), np.load(d / "crack_width" / "map_crack.npy")
    assert width.dtype == np.dtype("<f4") and crack.dtype == np.dtype("<i4") and label.dtype == np.uint8
    assert width.shape == crack.shape == label.shape == index.shape
    empty = index == 0xFFFFFFFF
    at = np.where(empty, 0, index).astype(np.int64)
    assert index[~empty].max() < len(map_width)
    assert width.tobytes() == np.where(empty, np.float32(0), map_width[at]).astype("<f4").tobytes()
    assert crack.tobytes() == np.where(empty, -1, map_crack[at]).astype("<i4").tobytes()
    assert (width > 0).sum() >= 20 and (crack >= 0).sum() >= 20, "cracks are drawn on the map"
    assert not label[empty].any() and len(np.unique(label)) >= 2


def test_streamed_files_are_the_one_shot_files(stream_dataset, tmp_path):  # noqa: F811
    common = ("--fuseMasks", "1", "--skip_filtered_dumps", "1", "--orthoMap", "1", "--orthoGsd", "0.01", "--orthoFill", "1")
    one = stream_cli._cli(stream_dataset, tmp_path / "one", *common, "--streamColour", "0")
    assert one.returncode == 0, one.stderr[-2000:]
    st = stream_cli._cli(stream_dataset, tmp_path / "streamed", *common, "--streamColour", "1", "--streamChunk", "4096")
    assert st.returncode == 0, st.stderr[-2000:]
    names = [k.split("/")[1] for k in NEW] + ["ortho_label.npy"]
    for name in names:
        a, b = (tmp_path / "one" / "ortho" / name).read_bytes(), (tmp_path / "streamed" / "ortho" / name).read_bytes()
        assert a == b, name
    meta = json.loads((tmp_path / "streamed" / "ortho" / "ortho_frame.json").read_text())
    assert meta["occupied"] > 1000 and meta["filled"] > 0 and meta["contributors"] > meta["occupied"]
    index = np.load(tmp_path / "streamed" / "ortho" / "ortho_index.npy")
    assert len(np.unique(np.load(tmp_path / "streamed" / "ortho" / "ortho_label.npy"))) >= 2
    # the index layer names rows of the whole smoothed cloud, not of a chunk
    m = re.search(r"^streamed colour: (\d+) chunks, (\d+) rows, (\d+) coloured$", st.stdout, re.M)
    assert m and int(m.group(1)) >= 4, st.stdout[-2000:]
    assert int(m.group(2)) // 2 < index[index != 0xFFFFFFFF].max() < int(m.group(2))


@pytest.mark.parametrize("flags, needles", [
    (("--orthoMap", "1", "--gpus", "2"), ("--orthoMap 1", "--gpus", "index shard", "not built")),
    (("--orthoMap", "1", "--orthoGsd", "2"), ("--orthoGsd", "invalid")),
    (("--orthoMap", "1", "--orthoFill", "2000"), ("--orthoFill", "invalid")),
    (("--orthoMap", "1", "--orthoFrame", "1,2,3"), ("--orthoFrame", "invalid")),
])
def test_refusals_name_the_flags(geometry_dataset, tmp_path, flags, needles):  # noqa: F811
    p = geometry_cli._cli(geometry_dataset, tmp_path / "out", *flags)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
