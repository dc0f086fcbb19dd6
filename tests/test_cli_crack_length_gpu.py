"""--crackLength 1 end to end ("Crack lengths on the map"): the three .npy files of the command line hold, bit for
bit, what capi's crack_lengths returns for the same map, poses and mask files, and crack_lengths_3d.json the table's integers
(its floats as "%.9g" prints them); cracks_3d.json and every other file are byte for byte those of a run with --crackFuse 1
alone; without --crackFuse 1, and where --crackFuse is refused, the run is refused with the reason."""
import json

import numpy as np
import pytest

from test_cli_crack_width_gpu import _cli, _files, dataset  # noqa: F401  (the wall patch, three keyframes, crack masks)

pytestmark = pytest.mark.gpu

W, H = 1024, 750
NEW = ["crack_width/map_crack_pos.npy", "crack_width/crack_paths.npy", "crack_width/crack_path_offsets.npy",
       "crack_width/crack_lengths_3d.json"]
UNIT = 1.0 / 1048576.0


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
        for k in range(len(ds["masks"])):
            ctx.crack_fuse_add(k, threshold, radius)
        out = ctx.crack_lengths(min_views, link)
        ctx.crack_fuse_end()
        return out
    finally:
        ctx.close()


def _g(v):
    return float("%.9g" % v)


def test_files_hold_the_librarys_arrays_and_nothing_else_changes(dataset, tmp_path):  # noqa: F811
    fused = _cli(dataset, tmp_path / "fused", "--crackFuse", "1", "--crackLength", "0", "--crackLinkRadius", "0.05")
    assert fused.returncode == 0, fused.stderr[-2000:]
    both = _cli(dataset, tmp_path / "both", "--crackFuse", "1", "--crackLength", "1", "--crackLinkRadius", "0.05", timing=tmp_path / "phases.json")
    assert both.returncode == 0, both.stderr[-2000:]
    a, c = _files(tmp_path / "fused"), _files(tmp_path / "both")
    assert "crack_width/cracks_3d.json" in a and not any(k in a for k in NEW)
    assert sorted(c) == sorted(list(a) + NEW)
    assert all(c[k] == a[k] for k in a), "cracks_3d.json and every other output file are byte for byte the same"
    n = len(dataset["pts"])
    want = _library(dataset, 0, 150, 1, 0.05)
    folder = tmp_path / "both" / "crack_width"
    for name, key, descr, shape in (("map_crack_pos", "pos", "<u8", (n,)), ("crack_paths", "path", "<i4", (want["path_points"],)),
                                    ("crack_path_offsets", "offsets", "<i8", (want["cracks"] + 1,))):
        got = np.load(folder / f"{name}.npy")
        assert got.dtype == np.dtype(descr) and got.shape == shape, name
        assert got.tobytes() == want[key].tobytes(), name
    rows = json.loads((folder / "crack_lengths_3d.json").read_text())
    assert len(rows) == want["cracks"] >= 1 and [r["id"] for r in rows] == [r["id"] for r in json.loads((folder / "cracks_3d.json").read_text())]
    assert (want["rows"][:, 3] > 0).any(), "no crack of more than one point: the scene is wrong"
    pts = dataset["pts"]
    for row, cid, r in zip(rows, want["ids"], want["rows"]):
        a_, b_, length_q, hops, sum_w, min_w, max_w = (int(v) for v in r)
        assert (row["id"], row["end_a"], row["end_b"], row["hops"]) == (int(cid), a_, b_, hops)
        assert row["length_m"] == _g(length_q * UNIT)
        assert row["end_a_xyz"] == [_g(v) for v in pts[a_]] and row["end_b_xyz"] == [_g(v) for v in pts[b_]]
        assert row["path_width_mean_mm"] == _g(sum_w / (hops + 1) * (1000.0 * UNIT))
        assert row["path_width_min_mm"] == _g(min_w * (1000.0 * UNIT)) and row["path_width_max_mm"] == _g(max_w * (1000.0 * UNIT))
    assert f"{want['cracks']} cracks, {want['path_points']} path points" in both.stdout
    phases = json.loads((tmp_path / "phases.json").read_text())  # the binary's own split
    assert phases["crack_length_gpu_s"] > 0 and phases["crack_length_write_s"] > 0 and phases["crack_fuse_gpu_s"] > 0


@pytest.mark.parametrize("flags, masks, needles", [
    (("--crackLength", "1"), True, ("--crackLength 1", "--crackFuse 1")),
    (("--crackFuse", "1", "--crackLength", "1"), False, ("--crackFuse 1", "--mask_image_folder")),
    (("--crackFuse", "1", "--crackLength", "1", "--gpus", "2"), True, ("--crackFuse 1", "--gpus", "index shard", "not built")),
    (("--crackFuse", "1", "--crackLength", "1", "--enableMLS", "1"), True, ("--crackFuse 1", "--enableMLS 1", "smoothed cloud")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, masks, needles):  # noqa: F811
    p = _cli(dataset, tmp_path / "out", *flags, masks=masks)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
