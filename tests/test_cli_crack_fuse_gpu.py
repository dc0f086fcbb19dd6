"""--crackFuse 1 / --crackLinkRadius r / --crackMinViews v end to end ("Crack widths on the map"): the four .npy
files of the command line hold, bit for bit, what capi's crack_fuse_fetch and crack_components return for the same map, poses
and mask files, and cracks_3d.json the table's integers (and its floats as "%.9g" prints them); every other output file is byte
for byte the file of a run without the flag; without --mask_image_folder, with --gpus 2 and with --enableMLS 1 the run is
refused with the reason."""
import json

import numpy as np
import pytest

from test_cli_crack_width_gpu import _cli, _files, dataset  # noqa: F401  (the wall patch, three keyframes, crack masks)

pytestmark = pytest.mark.gpu

W, H = 1024, 750
NEW = ["crack_width/map_width.npy", "crack_width/map_width_best.npy", "crack_width/map_views.npy", "crack_width/map_crack.npy",
       "crack_width/cracks_3d.json"]


def _library(ds, threshold, radius, min_views, link):
    from pointcloudprocessor_amd import capi

    ctx = capi.Context(0)
    try:
        cam = capi.default_camera()
        cam.image_width, cam.image_height = W, H
        ctx.set_camera(cam, capi.default_cull_params())
        pts = ds["pts"]
        ctx.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
        ctx.set_frames(ds["poses"])
        for k, m in enumerate(ds["masks"]):
            ctx.upload_mask(k, m)
        ctx.crack_fuse_begin()
        counts = [ctx.crack_fuse_add(k, threshold, radius) for k in range(len(ds["masks"]))]
        out = ctx.crack_fuse_fetch()
        out.update(ctx.crack_components(min_views, link))
        out["credited"] = sum(c[1] for c in counts)
        ctx.crack_fuse_end()
        return out
    finally:
        ctx.close()


def _g(v):
    return float("%.9g" % v)


def test_files_hold_the_librarys_arrays_and_nothing_else_changes(dataset, tmp_path):  # noqa: F811
    plain = _cli(dataset, tmp_path / "plain", "--crackFuse", "0", "--crackLinkRadius", "0.03", "--crackMinViews", "2")
    assert plain.returncode == 0, plain.stderr[-2000:]
    fused = _cli(dataset, tmp_path / "fused", "--crackFuse", "1", timing=tmp_path / "phases.json")
    assert fused.returncode == 0, fused.stderr[-2000:]
    other = _cli(dataset, tmp_path / "other", "--crackFuse", "1", "--crackPlaneRadius", "40", "--crackLinkRadius", "0.05", "--crackMinViews", "2")
    assert other.returncode == 0, other.stderr[-2000:]
    a, c, e = _files(tmp_path / "plain"), _files(tmp_path / "fused"), _files(tmp_path / "other")
    assert not any(k.startswith("crack_width/") for k in a)
    assert sorted(c) == sorted(list(a) + NEW) and sorted(e) == sorted(c)
    assert all(c[k] == a[k] for k in a) and all(e[k] == a[k] for k in a), "every other output file is byte for byte the same"
    n = len(dataset["pts"])
    for out, run, args in (("fused", fused, (0, 150, 1, 0.02)), ("other", other, (0, 40, 2, 0.05))):
        want = _library(dataset, *args)
        for name, key, descr in (("map_width", "width_mean", "<f4"), ("map_width_best", "width_best", "<f4"), ("map_views", "views", "<u4"),
                                 ("map_crack", "label", "<i4")):
            got = np.load(tmp_path / out / "crack_width" / f"{name}.npy")
            assert got.dtype == np.dtype(descr) and got.shape == (n,), name
            assert got.tobytes() == want[key].tobytes(), (out, name)
        rows = json.loads((tmp_path / out / "crack_width" / "cracks_3d.json").read_text())
        # (non-vacuity: the masks give more than 1000 width pixels -- test_cli_crack_width_gpu.py asserts it -- and the map has
        # 60 000 points over 768 000 pixels: some 80 credited points are to be expected, half of that is asked for)
        assert len(rows) == want["components"] >= 1 and (want["views"] > 0).sum() > 40
        if out == "fused":
            assert want["components"] > 1  # (several cracks at one view and 2 cm; two views and 5 cm may leave a single one)
        for row, cid, st, bx in zip(rows, want["ids"], want["stats"], want["box"]):
            assert (row["id"], row["points"], row["centre_points"]) == (int(cid), int(st[0]), int(st[4]))
            assert row["width_mean_mm"] == _g(int(st[1]) / int(st[0]) * (1000.0 / 1048576.0))
            assert row["width_min_mm"] == _g(int(st[2]) * (1000.0 / 1048576.0)) and row["width_max_mm"] == _g(int(st[3]) * (1000.0 / 1048576.0))
            assert row["box_min"] == [_g(v) for v in bx[:3]] and row["box_max"] == [_g(v) for v in bx[3:]]
            assert [np.float32(v) for v in row["box_min"] + row["box_max"]] == list(bx)
        assert f"{want['credited']} credited samples, {want['crack_points']} crack points, {want['components']} cracks" in run.stdout
    phases = json.loads((tmp_path / "phases.json").read_text())  # the binary's own split
    assert phases["crack_fuse_gpu_s"] > 0 and phases["crack_fuse_write_s"] > 0


def test_both_crack_outputs_share_the_folder(dataset, tmp_path):  # noqa: F811
    both = _cli(dataset, tmp_path / "both", "--crackWidth", "1", "--crackFuse", "1")
    assert both.returncode == 0, both.stderr[-2000:]
    files = _files(tmp_path / "both")
    assert all(k in files for k in NEW) and sum(k.endswith("_width.npy") and not k.endswith("map_width.npy") for k in files) == len(dataset["masks"])


@pytest.mark.parametrize("flags, masks, needles", [
    (("--crackFuse", "1"), False, ("--crackFuse 1", "--mask_image_folder")),
    (("--crackFuse", "1", "--gpus", "2"), True, ("--crackFuse 1", "--gpus", "index shard", "not built")),
    (("--crackFuse", "1", "--enableMLS", "1"), True, ("--crackFuse 1", "--enableMLS 1", "smoothed cloud")),
    (("--crackFuse", "1", "--crackLinkRadius", "0.004"), True, ("--crackLinkRadius", "invalid")),
    (("--crackFuse", "1", "--crackMinViews", "0"), True, ("--crackMinViews", "invalid")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, masks, needles):  # noqa: F811
    p = _cli(dataset, tmp_path / "out", *flags, masks=masks)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
