"""--balanceImages end to end: a run with --balanceImages 1 --claheClip 3 --balanceGamma 1.1 on the raw keyframe folder writes,
byte for byte, the PCDs of a run without the flag on a folder of keyframes pre-balanced with image_balance_host (PNG, so no
second lossy generation comes between); the same under the --gpus 2 rehearsal and with --streamColour 1; --balanceImages 0
is the run without the flag; the flag errors exit as the other options' do."""
import os
import subprocess

import numpy as np
import pytest

PIL = pytest.importorskip("PIL.Image")

pytestmark = pytest.mark.gpu

W, H = 1024, 750
FLAGS = ("--balanceImages", "1", "--claheClip", "3", "--balanceGamma", "1.1")
PARAMS = dict(stages=3, tiles=(8, 8), clip_limit=3.0, gamma=1.1)


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["PointCloudProcessor"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the scene of test_cli_stream_colour_gpu.py (a curved wall patch in view of six keyframes, stray points, points outside
    the crop box); raw/ holds the keyframes, balanced/ what image_balance_host makes of them"""
    from oracle import np_oracle as npo
    from pointcloudprocessor_amd import capi, synth

    d = tmp_path_factory.mktemp("image_balance")
    (d / "raw").mkdir()
    (d / "balanced").mkdir()
    rng = np.random.default_rng(21)
    poses, ts = synth.make_trajectory(6, spacing=0.12)
    n = 40_000
    p0 = poses[0, :3]
    R0 = npo.quat_to_rot(*poses[0, 3:7])  # camera -> world
    a, b = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    depth = 1.9 + 0.05 * np.sin(3.0 * a) + rng.normal(0, 1e-3, n)
    wall = p0 + a[:, None] * R0[:, 0] + b[:, None] * R0[:, 1] + depth[:, None] * R0[:, 2]
    stray = rng.uniform(-1.2, 1.2, (300, 3)) + p0 + 0.5 * R0[:, 2]
    far = rng.uniform(20, 30, (50, 3))
    pts = np.concatenate([wall, stray, far]).astype(np.float32)
    inten = rng.random(len(pts), dtype=np.float32)
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
            f"COUNT 1 1 1 1\nWIDTH {len(pts)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(pts)}\nDATA binary\n")
    with open(d / "scans.pcd", "wb") as f:
        f.write(head.encode())
        f.write(np.concatenate([pts, inten[:, None]], 1).astype("<f4").tobytes())
    changed = 0.0
    with open(d / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(ts, poses)):
            f.write(synth.odometry_line(t, p))
            bgr = (synth.make_image(k, W, H).astype(np.uint16) * 2 // 3).astype(np.uint8)  # darker: the balance has work to do
            bal = capi.image_balance_host(bgr, PARAMS)
            changed += float((bal != bgr).mean()) / len(ts)
            for folder, im in (("raw", bgr), ("balanced", bal)):  # (the reader goes by content: PNG under the .jpg name)
                PIL.fromarray(np.ascontiguousarray(im[:, :, ::-1])).save(d / folder / ("%f.jpg" % t), format="PNG")
    assert changed > 0.5
    return d


def _cli(ds, folder, out, *extra, env=None):
    out.mkdir()
    src = str(ds) + "/"
    cmd = [_exe(), "-p", src + "scans.pcd", "-o", src + "odo.txt", "-i", src + folder + "/", "-t", str(out) + "/"]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=out, env=env)


def _pcds(out):
    return {str(q.relative_to(out)): q.read_bytes() for q in sorted(out.rglob("*.pcd"))}


def _same_files(a, b):
    fa, fb = _pcds(a), _pcds(b)
    assert set(fa) == set(fb) and "cloudInWorldWithRGB.pcd" in fa and len(fa["cloudInWorldWithRGB.pcd"]) > 100_000
    for name in fa:
        assert fa[name] == fb[name], name
    return fa


def test_balanced_on_the_device_equals_prebalanced_folder(dataset, tmp_path):
    on = _cli(dataset, "raw", tmp_path / "on", *FLAGS)
    assert on.returncode == 0, on.stderr[-2000:]
    pre = _cli(dataset, "balanced", tmp_path / "pre")
    assert pre.returncode == 0, pre.stderr[-2000:]
    files = _same_files(tmp_path / "on", tmp_path / "pre")
    assert len(files) > 1 + 6, sorted(files)  # the final cloud and the per-keyframe dumps
    # --balanceImages 0 is the run without the flag, and not the balanced one
    off = _cli(dataset, "raw", tmp_path / "off", "--balanceImages", "0")
    assert off.returncode == 0, off.stderr[-2000:]
    plain = _cli(dataset, "raw", tmp_path / "plain")
    assert plain.returncode == 0, plain.stderr[-2000:]
    raw = _same_files(tmp_path / "off", tmp_path / "plain")
    assert raw["cloudInWorldWithRGB.pcd"] != files["cloudInWorldWithRGB.pcd"]


def test_two_gpu_rehearsal(dataset, tmp_path):
    env = dict(os.environ, PCP_MULTI_REHEARSAL="1")
    on = _cli(dataset, "raw", tmp_path / "on", *FLAGS, "--gpus", "2", env=env)
    assert on.returncode == 0, on.stderr[-2000:]
    pre = _cli(dataset, "balanced", tmp_path / "pre", "--gpus", "2", env=env)
    assert pre.returncode == 0, pre.stderr[-2000:]
    _same_files(tmp_path / "on", tmp_path / "pre")


def test_streamed_colour(dataset, tmp_path):
    mls = ("--enableMLS", "1", "--mlsVoxelSize", "0.004", "--mlsDilationIterations", "1", "--skip_filtered_dumps", "1", "--streamColour", "1",
           "--streamChunk", "4096")
    on = _cli(dataset, "raw", tmp_path / "on", *FLAGS, *mls)
    assert on.returncode == 0, on.stderr[-2000:]
    pre = _cli(dataset, "balanced", tmp_path / "pre", *mls)
    assert pre.returncode == 0, pre.stderr[-2000:]
    _same_files(tmp_path / "on", tmp_path / "pre")


@pytest.mark.parametrize("flags,names", [
    (("--balanceImages", "2"), ("'--balanceImages'", "is invalid (0, 1)")),
    (("--balanceImages", "1", "--claheClip", "-1"), ("'--claheClip'", "is invalid")),
    (("--balanceImages", "1", "--claheClip", "nan"), ("'--claheClip'", "is invalid")),
    (("--balanceImages", "1", "--claheTiles", "8"), ("'--claheTiles'", "is invalid (x,y with 1..16 each)")),
    (("--balanceImages", "1", "--claheTiles", "0,8"), ("'--claheTiles'", "is invalid")),
    (("--balanceImages", "1", "--claheTiles", "8,17"), ("'--claheTiles'", "is invalid")),
    (("--balanceImages", "1", "--balanceGamma", "0"), ("'--balanceGamma'", "is invalid")),
    (("--claheClip", "3"), ("'--claheClip'", "needs '--balanceImages 1'")),
    (("--claheTiles", "4,4", "--balanceImages", "0"), ("'--claheTiles'", "needs '--balanceImages 1'")),
    (("--balanceGamma", "1.1"), ("'--balanceGamma'", "needs '--balanceImages 1'")),
])
def test_flag_errors(dataset, tmp_path, flags, names):
    p = _cli(dataset, "raw", tmp_path / "out", *flags)
    assert p.returncode == 254, (p.returncode, p.stderr[-500:])
    for text in names:
        assert text in p.stderr, p.stderr[-1000:]
    assert not os.listdir(tmp_path / "out"), "refused before anything was read or written"
