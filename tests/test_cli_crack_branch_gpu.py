"""--crackBranches 1 / --crackPrune end to end ("Crack branches on the map"): the four .npy files of the command line
hold, bit for bit, what capi's crack_branches returns for the same map, poses and mask files, at the default prune and at a given
one, and crack_branches_3d.json what the tables, CB8 and crack_axis_host give (its floats as "%.9g" prints them); every other
file is byte for byte that of a run without the flag; a painted Y with a vertical, a horizontal and a diagonal arm comes out as
three branches of those classes; the refusals name the flags."""
import json

import numpy as np
import pytest

from test_cli_crack_direction_gpu import H, W, _context, _first_axes, _g, _klass, _stripe, _write_dataset
from test_cli_crack_width_gpu import _cli, _files, dataset  # noqa: F401  (the wall patch, three keyframes, crack masks)

pytestmark = pytest.mark.gpu

NEW = ["crack_width/map_crack_branch.npy", "crack_width/crack_branches.npy", "crack_width/crack_branch_ids.npy",
       "crack_width/crack_branch_moments.npy", "crack_width/crack_branches_3d.json"]
WORDS = ("branch_count", "bridges", "junctions_kept", "ends_kept", "pruned_branches", "pruned_nodes", "pruned_points")
UNIT = 2.0 ** -20


def _library(ds, link, step, prune):
    ctx = _context(ds["pts"], ds["poses"], ds["masks"])
    try:
        ctx.crack_fuse_begin()
        for k in range(len(ds["masks"])):
            ctx.crack_fuse_add(k, 0, 150)
        out = ctx.crack_branches(1, link, step, prune)
        ctx.crack_fuse_end()
        return out
    finally:
        ctx.close()


def _check_files(folder, want, n, up):
    for name, key, dtype, shape in (("map_crack_branch", "branch", "<i4", (n,)), ("crack_branches", "rows", "<i8", (len(want["ids"]), 15)),
                                    ("crack_branch_ids", "ids", "<i4", (len(want["ids"]),)),
                                    ("crack_branch_moments", "moments", "<i8", (len(want["ids"]), 20))):
        got = np.load(folder / f"{name}.npy")
        assert got.dtype == np.dtype(dtype) and got.shape == shape and got.tobytes() == want[key].tobytes(), name
    recs = json.loads((folder / "crack_branches_3d.json").read_text())
    assert len(recs) == len(want["cracks"]) >= 1 and [r["id"] for r in recs] == [r["id"] for r in json.loads((folder / "cracks_3d.json").read_text())]
    rows = want["rows"]
    for r, rec in enumerate(recs):
        assert set(rec) == {"id", "kept_length_m", "branches"} | set(WORDS)
        assert [rec[k] for k in WORDS] == want["cracks"][r].tolist() and rec["kept_length_m"] == _g(want["kept_length_m"][r])
        mine = np.flatnonzero(rows[:, 0] == r)
        assert len(rec["branches"]) == len(mine) == rec["branch_count"]
        for b, br in zip(mine.tolist(), rec["branches"]):
            assert set(br) == {"id", "points", "length_m", "mean_width", "min_width", "max_width", "arc_from_m", "arc_to_m", "attachments",
                               "centroid", "axis", "anisotropy", "inclination_deg", "class"}
            assert (br["id"], br["points"], br["attachments"]) == (int(want["ids"][b]), int(rows[b, 6]), int(rows[b, 3]))
            assert br["length_m"] == _g(want["length_m"][b]) and br["mean_width"] == _g(want["mean_width"][b])  # CB8
            assert br["min_width"] == _g(rows[b, 8] * UNIT) and br["max_width"] == _g(rows[b, 9] * UNIT)
            assert br["arc_from_m"] == _g(rows[b, 10] * UNIT) and br["arc_to_m"] == _g(rows[b, 11] * UNIT)
            assert br["centroid"] == [_g(v) for v in want["centroid"][b]]
            assert br["axis"] == [_g(v) for v in want["axis"][b]] and br["anisotropy"] == _g(want["anisotropy"][b])  # crack_axis_host
            incl, cls = _klass(want["axis"][b], up)
            assert abs(br["inclination_deg"] - incl) <= 1e-6
            if min(abs(incl - 22.5), abs(incl - 67.5)) > 1e-6:
                assert br["class"] == cls
    return recs


def test_files_hold_the_librarys_arrays_and_nothing_else_changes(dataset, tmp_path):  # noqa: F811
    up = np.array([0.0, 0.0, 1.0])
    base = ("--crackFuse", "1", "--crackLength", "1", "--crackLinkRadius", "0.05")
    fused = _cli(dataset, tmp_path / "fused", *base)
    assert fused.returncode == 0, fused.stderr[-2000:]
    plain = _cli(dataset, tmp_path / "plain", *base, "--crackBranches", "1", timing=tmp_path / "phases.json")
    assert plain.returncode == 0, plain.stderr[-2000:]
    given = _cli(dataset, tmp_path / "given", *base, "--crackBranches", "1", "--crackPrune", "0.35", "--crackSkeletonStep", "0.07")
    assert given.returncode == 0, given.stderr[-2000:]
    a, c, e = _files(tmp_path / "fused"), _files(tmp_path / "plain"), _files(tmp_path / "given")
    assert "crack_width/cracks_3d.json" in a and not any(k in a for k in NEW)
    assert sorted(c) == sorted(list(a) + NEW) == sorted(e), "the skeleton is made, its files are not written"
    assert all(c[k] == a[k] for k in a) and all(e[k] == a[k] for k in a), "every other output file is byte for byte the same"
    n = len(dataset["pts"])
    step = float(np.float32(2.0) * np.float32(0.05))
    want = _library(dataset, 0.05, None, float(np.float32(2.0) * np.float32(step)))  # the defaults: a band of two radii, prune two bands
    recs = _check_files(tmp_path / "plain" / "crack_width", want, n, up)
    assert sum(len(r["branches"]) for r in recs) == len(want["ids"]) >= len(recs)  # (these cracks are 0.1 m long: the forks are the painted Y's)
    assert f"{len(want['cracks'])} cracks, {len(want['ids'])} branches, {want['pruned_branches']} pruned" in plain.stdout
    other = _library(dataset, 0.05, 0.07, 0.35)
    _check_files(tmp_path / "given" / "crack_width", other, n, up)
    print("default:", len(want["ids"]), "branches,", want["pruned_branches"], "pruned; step 0.07, prune 0.35:", len(other["ids"]), "branches,",
          other["pruned_branches"], "pruned")
    phases = json.loads((tmp_path / "phases.json").read_text())  # the binary's own split
    assert phases["crack_branches_gpu_s"] > 0 and phases["crack_branches_write_s"] > 0 and phases["crack_fuse_gpu_s"] > 0
    assert "crack_skeleton_gpu_s" not in phases and "crack_skeleton_write_s" not in phases


def test_a_painted_y_has_three_branches_of_the_painted_classes(tmp_path):
    """one keyframe before the slanted wall of the direction test with three stripes from one point: up the image, across it, and
    down to the left at 45 degrees.  With the camera's down axis as --crackUp its three branches are vertical, horizontal and
    diagonal, where the crack's one axis is none of them."""
    poses, ts, p0, R0 = _first_axes()
    rng = np.random.default_rng(71)
    n = 300_000
    a, b = rng.uniform(-0.95, -0.3, n), rng.uniform(-0.7, -0.25, n)
    depth = 1.9 + 0.2 * a + rng.normal(0, 5e-4, n)
    pts = (p0 + a[:, None] * R0[:, 0] + b[:, None] * R0[:, 1] + depth[:, None] * R0[:, 2]).astype(np.float32)
    mask = np.zeros((H, W), np.uint8)
    _stripe(mask, 560, 380, 560, 60, 8)
    _stripe(mask, 560, 380, 980, 380, 8)
    _stripe(mask, 560, 380, 260, 680, 8)
    ds = _write_dataset(tmp_path, pts, poses, ts, [mask])
    up = R0[:, 1]
    run = _cli(ds, tmp_path / "run", "--crackFuse", "1", "--crackBranches", "1", "--crackDirection", "1", "--crackUp",
               ",".join(repr(float(v)) for v in up))
    assert run.returncode == 0, run.stderr[-2000:]
    folder = tmp_path / "run" / "crack_width"
    recs = json.loads((folder / "crack_branches_3d.json").read_text())
    whole = {r["id"]: r for r in json.loads((folder / "crack_directions_3d.json").read_text())}
    rec = max(recs, key=lambda r: sum(b["points"] for b in r["branches"]))
    arms = sorted(rec["branches"], key=lambda b: -b["length_m"])
    print({k: rec[k] for k in WORDS}, [(b["id"], b["points"], b["length_m"], b["class"], b["inclination_deg"], b["attachments"]) for b in arms],
          whole[rec["id"]]["class"], whole[rec["id"]]["inclination_deg"])
    assert rec["branch_count"] == 3 and rec["junctions_kept"] == 1 and rec["ends_kept"] == 3, "the Y is not a Y: the scene is wrong"
    got = {b["class"]: b for b in arms}
    assert set(got) == {"vertical", "horizontal", "diagonal"}
    assert got["vertical"]["inclination_deg"] < 5.0 and got["horizontal"]["inclination_deg"] > 85.0
    assert abs(got["diagonal"]["inclination_deg"] - np.degrees(np.arccos(1.0 / np.sqrt(2.04)))) < 5.0
    assert all(b["attachments"] == 1 and b["anisotropy"] > 0.9 and b["length_m"] > 0.05 for b in arms)
    assert abs(sum(b["length_m"] for b in arms) - rec["kept_length_m"]) <= 1e-6  # (no bridge: every kept edge belongs to an arm)
    # a given prune above every arm: the arm that holds neither end of the stem goes, the junction dissolves; the files are capi's
    far = _cli(ds, tmp_path / "far", "--crackFuse", "1", "--crackBranches", "1", "--crackPrune", "1", "--crackUp", ",".join(repr(float(v)) for v in up))
    assert far.returncode == 0, far.stderr[-2000:]
    want = _library(ds, 0.02, None, 1.0)
    pruned = _check_files(tmp_path / "far" / "crack_width", want, len(pts), up)
    one = next(r for r in pruned if r["id"] == rec["id"])
    print({k: one[k] for k in WORDS}, [(b["id"], b["points"], b["length_m"], b["class"]) for b in one["branches"]])
    assert (one["branch_count"], one["junctions_kept"], one["ends_kept"], one["pruned_branches"]) == (1, 0, 2, 1) and one["pruned_points"] > 0
    assert one["kept_length_m"] < rec["kept_length_m"] and (np.load(tmp_path / "far" / "crack_width" / "map_crack_branch.npy") == -3).sum() == \
        sum(r["pruned_points"] for r in pruned)


@pytest.mark.parametrize("flags, masks, needles", [
    (("--crackBranches", "1"), True, ("--crackBranches 1", "--crackFuse 1")),
    (("--crackFuse", "1", "--crackBranches", "1", "--crackPrune", "-0.5"), True, ("--crackPrune", "1024")),
    (("--crackFuse", "1", "--crackBranches", "1", "--crackPrune", "1025"), True, ("--crackPrune", "1024")),
    (("--crackFuse", "1", "--crackBranches", "1", "--crackPrune", "nan"), True, ("--crackPrune", "1024")),
    (("--crackFuse", "1", "--crackBranches", "1", "--crackSkeletonStep", "17"), True, ("--crackSkeletonStep",)),
    (("--crackFuse", "1", "--crackBranches", "1"), False, ("--crackFuse 1", "--mask_image_folder")),
    (("--crackFuse", "1", "--crackBranches", "1", "--gpus", "2"), True, ("--crackFuse 1", "--gpus", "index shard", "not built")),
])
def test_refusals_name_the_flags(dataset, tmp_path, flags, masks, needles):  # noqa: F811
    p = _cli(dataset, tmp_path / "out", *flags, masks=masks)
    assert p.returncode == 254, (p.returncode, p.stderr[-1000:])  # main's -2
    for s in needles:
        assert s in p.stderr, p.stderr[-1000:]
    assert not list((tmp_path / "out").iterdir()), "refused before anything was read or written"
