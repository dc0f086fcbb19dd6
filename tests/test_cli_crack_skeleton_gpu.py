"""--crackSkeleton 1 end to end ("Crack skeletons on the map"): the four .npy files of the command line hold, bit for
bit, what capi's crack_skeleton returns for the same map, poses and mask files, and crack_skeleton_3d.json the summary's integers
and CS7's metres (as "%.9g" prints them); every other file is byte for byte that of a run with --crackFuse 1 alone, and a run
without the flag writes the file list it wrote before; without --crackFuse 1, and where --crackFuse is refused, the run is
refused with the reason."""
import json

import numpy as np
import pytest

from test_cli_crack_length_gpu import H, W, _g
from test_cli_crack_width_gpu import _cli, _files, dataset  # noqa: F401  (the wall patch, three keyframes, crack masks)

pytestmark = pytest.mark.gpu

NEW = ["crack_width/map_crack_node.npy", "crack_width/crack_nodes.npy", "crack_width/crack_node_ids.npy", "crack_width/crack_edges.npy",
       "crack_width/crack_skeleton_3d.json"]
FUSED = ["crack_width/map_width.npy", "crack_width/map_width_best.npy", "crack_width/map_views.npy", "crack_width/map_crack.npy",
         "crack_width/cracks_3d.json"]  # what --crackFuse 1 alone adds to a run, before and after this flag existed


def _library(ds, threshold, radius, min_views, link, step):
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
        out = ctx.crack_skeleton(min_views, link, step)
        ctx.crack_fuse_end()
        return out
    finally:
        ctx.close()


def test_files_hold_the_librarys_arrays_and_nothing_else_changes(dataset, tmp_path):  # noqa: F811
    fused = _cli(dataset, tmp_path / "fused", "--crackFuse", "1", "--crackSkeleton", "0", "--crackLinkRadius", "0.05")
    assert fused.returncode == 0, fused.stderr[-2000:]
    both = _cli(dataset, tmp_path / "both", "--crackFuse", "1", "--crackSkeleton", "1", "--crackLinkRadius", "0.05", timing=tmp_path / "phases.json")
    assert both.returncode == 0, both.stderr[-2000:]
    stepped = _cli(dataset, tmp_path / "stepped", "--crackFuse", "1", "--crackSkeleton", "1", "--crackLinkRadius", "0.05", "--crackSkeletonStep", "0.0625")
    assert stepped.returncode == 0, stepped.stderr[-2000:]
    a, c, d = _files(tmp_path / "fused"), _files(tmp_path / "both"), _files(tmp_path / "stepped")
    assert sorted(k for k in a if k.startswith("crack_width/")) == sorted(FUSED), "a run without the flag writes the files it wrote before"
    assert sorted(c) == sorted(list(a) + NEW) and sorted(d) == sorted(c)
    assert all(c[k] == a[k] for k in a) and all(d[k] == a[k] for k in a), "every other output file is byte for byte the same"
    n = len(dataset["pts"])
    for run, step, stdout in (("both", None, both.stdout), ("stepped", 0.0625, stepped.stdout)):
        want = _library(dataset, 0, 150, 1, 0.05, step)
        kn, ke, kc = len(want["ids"]), len(want["edges"]), len(want["cracks"])
        folder = tmp_path / run / "crack_width"
        for name, key, descr, shape in (("map_crack_node", "node", "<i4", (n,)), ("crack_nodes", "nodes", "<i8", (kn, 10)),
                                        ("crack_node_ids", "ids", "<i4", (kn,)), ("crack_edges", "edges", "<i8", (ke, 3))):
            got = np.load(folder / f"{name}.npy")
            assert got.dtype == np.dtype(descr) and got.shape == shape, (run, name)
            assert got.tobytes() == want[key].tobytes(), (run, name)
        rows = json.loads((folder / "crack_skeleton_3d.json").read_text())
        assert len(rows) == kc >= 1 and [r["id"] for r in rows] == [r["id"] for r in json.loads((folder / "cracks_3d.json").read_text())]
        if step is not None:
            assert (want["cracks"][:, 1] > 0).any(), "no crack of more than one node: the scene is wrong"
        nodes, centroids = want["nodes"], want["centroids"]
        for r, (row, c6) in enumerate(zip(rows, want["cracks"])):
            assert [row[k] for k in ("nodes", "edges", "ends", "junctions", "loops")] == [int(v) for v in c6[:5]]
            assert row["skeleton_length_m"] == _g(want["skeleton_length_m"][r])
            mine = nodes[:, 0] == r
            assert row["end_xyz"] == [[_g(v) for v in centroids[k]] for k in np.flatnonzero(mine & (nodes[:, 9] == 1))]
            assert row["junction_xyz"] == [[_g(v) for v in centroids[k]] for k in np.flatnonzero(mine & (nodes[:, 9] >= 3))]
        assert f"{kc} cracks, {kn} nodes, {ke} edges" in stdout
    phases = json.loads((tmp_path / "phases.json").read_text())  # the binary's own split
    assert phases["crack_skeleton_gpu_s"] > 0 and phases["crack_skeleton_write_s"] > 0 and phases["crack_fuse_gpu_s"] > 0


@pytest.mark.parametrize("flags, masks, needles", [
    (("--crackSkeleton", "1"), True, ("--crackSkeleton 1", "--crackFuse 1")),
    (("--crackFuse", "1", "--crackSkeleton", "1", "--crackSkeletonStep", "17"), True, ("--crackSkeletonStep", "16")),
    (("--crackFuse", "1", "--crackSkeleton", "1"), False, ("--crackFuse 1", "--mask_image_folder")),
    (("--crackFuse", "1", "--crackSkeleton", "1", "--gpus", "2"), True, ("--crackFuse 1", "--gpus", "index shard", "not built")),
    (("--crackFuse", "1", "--crackSkeleton", "1", "--enableMLS", "1"), True, ("--crackFuse 1", "--enableMLS 1", "smoothed cloud")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, masks, needles):  # noqa: F811
    p = _cli(dataset, tmp_path / "out", *flags, masks=masks)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
