"""smoothColorsWithLocalRegion on the MI355X (csrc/pcp_colour_smooth.hip) against the restatement of DESIGN.md LS1-LS7
(tests/_local_smooth_ref.py), bit for bit: the packed and in-place forms, order invariance, degenerate clouds, the full-size
map, the command line and the C++ shim."""
import os
import subprocess

import numpy as np
import pytest

import _local_smooth_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu


def _words(rng, n, zero_share=0.2):
    w = rng.integers(0, 1 << 25, n, dtype=np.uint32)  # colours and a random has bit
    w[rng.random(n) < zero_share] = 0
    return w


def _sample(n, k, seed=0):
    if n <= k:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False))


def _check_packed(ctx, x, y, z, words, radius, sample=20000):
    out, has_count = ctx.colour_smooth_local_packed(radius, words)
    assert has_count == int(((out >> 24) & 1).sum())
    q = _sample(len(x), sample)
    want = ref.smooth_local(x, y, z, words, radius, queries=q)
    bad = np.nonzero(out[q] != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(q)} differ, first {q[bad[:5]]}: got {out[q[bad[:5]]]}, want {want[bad[:5]]}"
    return out


@pytest.mark.parametrize("n,radius", [(20_000, 0.1), (20_000, 0.02), (20_000, 1e-3), (200_000, 0.1), (200_000, 0.02),
                                      (200_000, 1e-3), (200_000, 0.5), (1_000_000, 0.1), (1_000_000, 0.02),
                                      (1_000_000, 1e-3)])
def test_packed_form_equals_restatement(gpu_ctx_factory, n, radius):
    from pointcloudprocessor_amd import synth

    x, y, z, _ = synth.make_cloud(n, seed=31)
    words = _words(np.random.default_rng(n), n)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    _check_packed(ctx, x, y, z, words, radius, sample=n if n <= 20_000 else 20_000)


def test_packed_form_in_device_memory_and_in_place(gpu_ctx_factory):
    import torch

    from pointcloudprocessor_amd import capi, synth

    n = 50_000
    x, y, z, _ = synth.make_cloud(n, seed=4)
    words = _words(np.random.default_rng(4), n)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    want, want_count = ctx.colour_smooth_local_packed(0.1, words)
    d = torch.from_numpy(words.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    import ctypes as C

    cnt = C.c_int64()
    rc = ctx.lib.pcp_colour_smooth_local_packed(ctx.h, C.c_float(0.1), C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()),
                                                C.byref(cnt))
    assert rc == capi.PCP_OK
    assert np.array_equal(d.cpu().numpy().view(np.uint32), want) and cnt.value == want_count


def _colour_context(gpu_ctx_factory, sc, cull_mode=None):
    from pointcloudprocessor_amd import capi

    ctx = gpu_ctx_factory()
    cull = capi.default_cull_params()
    if cull_mode is not None:
        cull.cull_mode = cull_mode
    ctx.set_camera(capi.camera_from_dict(sc["cam"]), cull)
    ctx.upload_cloud(sc["x"], sc["y"], sc["z"])
    ctx.set_frames(sc["poses"])
    for f, im in enumerate(sc["images"]):
        ctx.upload_image(f, im)
    return ctx


def _device_words(ctx):
    import torch

    from pointcloudprocessor_amd.pipeline import _DeviceArray

    ptr, n = ctx.colour_result_device()
    ctx.synchronize()
    return torch.as_tensor(_DeviceArray(ptr, n, "<u4"), device="cuda:0").cpu().numpy().copy()


def test_in_place_after_colorize(gpu_ctx_factory, small_scene):
    import torch

    from pointcloudprocessor_amd import capi

    sc = small_scene
    ctx = _colour_context(gpu_ctx_factory, sc)
    import ctypes as C

    cnt = C.c_int64()
    assert ctx.lib.pcp_colour_smooth_local(ctx.h, C.c_float(0.1), C.byref(cnt)) == capi.PCP_ERR_STATE  # no result yet
    ctx.colorize()
    before = ctx.download_result_packed()
    # an asynchronous download of the unsmoothed words is still in flight when the pass runs
    pinned = torch.empty(ctx.n, dtype=torch.int32).pin_memory()
    ctx.download_result_packed_async(pinned.data_ptr())
    has_count = ctx.colour_smooth_local(0.1)
    ctx.synchronize()
    assert np.array_equal(pinned.numpy().view(np.uint32), before)
    want = ref.smooth_local(sc["x"], sc["y"], sc["z"], before, 0.1)
    got = ctx.download_result_packed()
    assert np.array_equal(got, want)
    assert has_count == int(((want >> 24) & 1).sum())
    assert int(((want >> 24) & 1).sum()) >= int(((before >> 24) & 1).sum())
    assert np.array_equal(_device_words(ctx), want)
    pinned2 = torch.empty(ctx.n, dtype=torch.int32).pin_memory()
    ctx.download_result_packed_async(pinned2.data_ptr())
    ctx.synchronize()
    assert np.array_equal(pinned2.numpy().view(np.uint32), want)
    # the next colour run starts from the unsmoothed colours again
    ctx.colorize()
    assert np.array_equal(ctx.download_result_packed(), before)


def test_in_place_after_finalise_with_hpr(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    sc = small_scene
    ctx = _colour_context(gpu_ctx_factory, sc, capi.CULL_HPR)
    ctx.colour_reset()
    ctx.depth_pass()
    ctx.colour_pass()
    ctx.colour_finalise()
    before = ctx.download_result_packed()
    has_count = ctx.colour_smooth_local(0.05)
    want = ref.smooth_local(sc["x"], sc["y"], sc["z"], before, 0.05)
    assert np.array_equal(ctx.download_result_packed(), want)
    assert np.array_equal(_device_words(ctx), want)
    assert has_count == int(((want >> 24) & 1).sum())


def test_order_invariance(gpu_ctx_factory):
    from pointcloudprocessor_amd import synth

    n = 100_000
    x, y, z, _ = synth.make_cloud(n, seed=8)
    words = _words(np.random.default_rng(8), n)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    a, ca = ctx.colour_smooth_local_packed(0.1, words)
    p = np.random.default_rng(9).permutation(n)
    ctx.upload_cloud(x[p], y[p], z[p])
    b, cb = ctx.colour_smooth_local_packed(0.1, words[p])
    assert np.array_equal(b, a[p]) and ca == cb


def test_all_duplicates_overflow_one_tile(gpu_ctx_factory):
    n = 50_000
    x = np.full(n, 1.25, np.float32)
    y = np.full(n, -3.5, np.float32)
    z = np.full(n, 0.75, np.float32)
    words = _words(np.random.default_rng(3), n)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    out, cnt = ctx.colour_smooth_local_packed(0.1, words)
    r, g, b = ref.split(words)
    want = ref.pack(r.sum() // n, g.sum() // n, b.sum() // n)  # every w is 1
    assert np.all(out == want) and cnt == (n if (want >> 24) & 1 else 0)


def test_stray_point_far_away(gpu_ctx_factory):
    from pointcloudprocessor_amd import synth

    n = 20_000
    x, y, z, _ = synth.make_cloud(n, seed=12)
    x[17] = np.float32(1000.0)
    words = _words(np.random.default_rng(12), n)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    out = _check_packed(ctx, x, y, z, words, 0.1, sample=n)
    assert out[17] == ref.pack(*(int(v[17]) for v in ref.split(words)))


def test_one_and_zero_points(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    one = np.array([0.5], np.float32)
    ctx.upload_cloud(one, one, one)
    out, cnt = ctx.colour_smooth_local_packed(0.1, np.array([0x00102030], np.uint32))
    assert out[0] == 0x01102030 and cnt == 1
    out, cnt = ctx.colour_smooth_local_packed(0.1, np.array([0x01000000], np.uint32))
    assert out[0] == 0 and cnt == 0
    empty = np.zeros(0, np.float32)
    ctx.upload_cloud(empty, empty, empty)
    out, cnt = ctx.colour_smooth_local_packed(0.1, np.zeros(0, np.uint32))
    assert len(out) == 0 and cnt == 0


def test_non_finite_points(gpu_ctx_factory):
    from pointcloudprocessor_amd import synth

    n = 30_000
    x, y, z, _ = synth.make_cloud(n, seed=14)
    rng = np.random.default_rng(14)
    x[rng.random(n) < 0.02] = np.nan
    y[rng.random(n) < 0.01] = np.inf
    z[rng.random(n) < 0.01] = -np.inf
    words = _words(rng, n)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    out = _check_packed(ctx, x, y, z, words, 0.1, sample=n)
    bad = ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
    assert np.array_equal(out[bad], words[bad])
    # every point non-finite: nothing changes
    ctx.upload_cloud(np.full(10, np.nan, np.float32), y[:10], z[:10])
    out, cnt = ctx.colour_smooth_local_packed(0.1, words[:10])
    assert np.array_equal(out, words[:10]) and cnt == int(((words[:10] >> 24) & 1).sum())


def test_one_cell_of_65_finite_points_and_a_nan(gpu_ctx_factory):
    """one full work item of 64 queries plus one, through the gathered view of the finite points"""
    rng = np.random.default_rng(65)
    x, y, z = (np.float32(c) + rng.random(66).astype(np.float32) * np.float32(0.05) for c in (1.0, -2.0, 0.5))
    y[40] = np.nan
    words = _words(rng, 66, zero_share=0.0)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    out = _check_packed(ctx, x, y, z, words, 0.1, sample=66)
    assert out[40] == words[40]


def test_radius_rules(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi

    ctx = gpu_ctx_factory()
    one = np.array([0.5, 0.6], np.float32)
    ctx.upload_cloud(one, one, one)
    for r in (0.0, -0.1, 1.0001, float("nan"), float("inf")):
        with pytest.raises(capi.PcpError) as e:
            ctx.colour_smooth_local_packed(r, np.zeros(2, np.uint32))
        assert e.value.code == capi.PCP_ERR_INVALID
    ctx.colour_smooth_local_packed(1.0, np.zeros(2, np.uint32))


def test_full_size_map_sampled(gpu_ctx_factory):
    from pointcloudprocessor_amd import synth

    n = 10_000_000
    x, y, z, _ = synth.make_cloud(n)
    words = _words(np.random.default_rng(10), n)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    _check_packed(ctx, x, y, z, words, 0.1, sample=20_000)


def test_pipeline_engine(small_scene):
    from pointcloudprocessor_amd import pipeline

    sc = small_scene
    eng = pipeline.HipEngine(0)
    try:
        eng.configure(sc["cam"])
        eng.upload_cloud(sc["x"], sc["y"], sc["z"])
        eng.set_keyframes(sc["poses"], sc["images"])
        col = pipeline.PointCloudColorizer(eng)
        plain = col.run()
        words = plain["rgb"][:, 0].astype(np.uint32) | (plain["rgb"][:, 1].astype(np.uint32) << 8) | (
            plain["rgb"][:, 2].astype(np.uint32) << 16)
        smoothed = col.run(local_smooth_radius=0.1)
        want = ref.smooth_local(sc["x"], sc["y"], sc["z"], words, 0.1)
        r, g, b = ref.split(want)
        assert np.array_equal(smoothed["rgb"], np.stack([r, g, b], 1).astype(np.uint8))
        assert np.array_equal(smoothed["has"], ((want >> 24) & 1).astype(np.uint8))
    finally:
        eng.close()


# ---- command line --------------------------------------------------------------------------------------------------


def _cli_scene(tmp_path, n=60000, W=1024, H=750):
    from PIL import Image

    from pointcloudprocessor_amd import synth
    from test_cli import _write_pcd_binary

    x, y, z, inten = synth.make_cloud(n, seed=9)
    _write_pcd_binary(tmp_path / "scans.pcd", x, y, z, inten)
    poses, ts = synth.make_trajectory(10, spacing=0.06)
    with open(tmp_path / "odo.txt", "w") as f:
        for k, (t, p) in enumerate(zip(ts, poses)):
            f.write(synth.odometry_line(t, p))
            Image.fromarray(synth.make_image(k, W, H)[:, :, ::-1]).save(tmp_path / ("%f.jpg" % t), quality=92)
            Image.fromarray(synth.make_mask(k, W, H)).save(tmp_path / ("%f.png" % t))
    return x, y, z


def _run_cli(tmp_path, name, extra, env=None):
    from test_cli import _exe

    d = tmp_path / name
    d.mkdir()
    src = str(tmp_path) + "/"
    p = subprocess.run([_exe(), "-p", str(tmp_path / "scans.pcd"), "-o", str(tmp_path / "odo.txt"), "-i", src, "-m", src,
                        "-t", str(d) + "/"] + extra, capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return d


def _rows_words(path):
    from test_cli import _read_pcd_ascii

    _, rows = _read_pcd_ascii(path)
    xyz = np.array([[np.float32(float(v)) for v in r[:3]] for r in rows], np.float32).reshape(-1, 3)
    rgb = np.array([int(r[3]) for r in rows], np.uint64)
    return xyz, rgb


def test_cli_smooth_colors_radius(tmp_path):
    x, y, z = _cli_scene(tmp_path)
    plain = _run_cli(tmp_path, "plain", [])
    timing = tmp_path / "timing.json"
    env = dict(os.environ, PCP_CLI_TIMING=str(timing))
    smooth = _run_cli(tmp_path, "smooth", ["--smoothColorsRadius", "0.1"], env=env)
    import json

    assert "colour_smooth_gpu_s" in json.loads(timing.read_text())
    # every other file is byte-identical
    names = sorted(str(q.relative_to(plain)) for q in plain.rglob("*.pcd"))
    assert names == sorted(str(q.relative_to(smooth)) for q in smooth.rglob("*.pcd"))
    for name in names:
        if name != "cloudInWorldWithRGB.pcd":
            assert (plain / name).read_bytes() == (smooth / name).read_bytes(), name
    # the unsmoothed words of the one-GPU run: the coloured rows of the plain file, (0, 0, 0) elsewhere (LS1); the rows are
    # the coloured points in input order, so they are matched to the cloud by position
    pxyz, prgb = _rows_words(plain / "cloudInWorldWithRGB.pcd")
    pts = np.stack([x, y, z], 1)
    from scipy.spatial import cKDTree

    tree = cKDTree(pts.astype(np.float64))
    d, idx = tree.query(pxyz.astype(np.float64))
    assert np.all(d < 1e-5) and len(np.unique(idx)) == len(idx)
    words = np.zeros(len(x), np.uint32)
    words[idx] = ((prgb >> 16) & 0xFF).astype(np.uint32) | (((prgb >> 8) & 0xFF).astype(np.uint32) << 8) | (
        (prgb & 0xFF).astype(np.uint32) << 16) | (1 << 24)
    want = ref.smooth_local(x, y, z, words, 0.1)
    sel = np.nonzero((want >> 24) & 1)[0]
    sxyz, srgb = _rows_words(smooth / "cloudInWorldWithRGB.pcd")
    assert len(srgb) == len(sel) >= len(prgb)
    assert np.array_equal(tree.query(sxyz.astype(np.float64))[1], sel)
    r, g, b = ref.split(want[sel])
    assert np.array_equal(srgb, (0xFF000000 | (r.astype(np.uint64) << 16) | (g.astype(np.uint64) << 8) | b.astype(np.uint64)))
    # three index shards (rehearsal on one device): the same bytes as one GPU
    env3 = dict(os.environ, PCP_MULTI_REHEARSAL="1")
    three = _run_cli(tmp_path, "three", ["--smoothColorsRadius", "0.1", "--gpus", "3"], env=env3)
    for name in names:
        assert (smooth / name).read_bytes() == (three / name).read_bytes(), name


# ---- C++ shim --------------------------------------------------------------------------------------------------------

_SHIM_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "pcp_shim.hpp"
int main() {
  try {
    pcp_amd::Device dev(0);
    pcp_camera cam;
    pcp_default_camera(&cam);
    cam.fx = cam.fy = 188.2083; cam.cx = 80.0; cam.cy = 45.0;
    cam.image_width = cam.cull_width = 160; cam.image_height = cam.cull_height = 90;
    dev.setCamera(cam);
    const int n = 4000;
    std::vector<float> x(n), y(n), z(n);
    unsigned s = 777u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return static_cast<float>(s >> 8) / 16777216.0f; };
    for (int i = 0; i < n; ++i) { x[i] = (rnd() - 0.5f) * 3.0f; y[i] = (rnd() - 0.5f) * 1.6f; z[i] = 3.0f; }
    dev.uploadCloud(x.data(), y.data(), z.data(), n);
    std::vector<pcp_pose> poses(2, pcp_pose{0, 0, 0, 1, 0, 0, 0});
    poses[1].x = 0.05;
    dev.setKeyframes(poses);
    std::vector<uint8_t> img(160 * 90 * 3);
    for (int f = 0; f < 2; ++f) {
      for (size_t i = 0; i < img.size(); ++i) img[i] = static_cast<uint8_t>((i * 7 + f * 31) % 251 + 1);
      dev.uploadImage(f, img.data(), 160 * 3);
    }
    pcp_amd::Colorizer c(dev);
    std::vector<uint8_t> rgb, has, rgb2, has2;
    c.colorize(rgb, has);
    const long long coloured = static_cast<long long>(c.smoothColorsWithLocalRegion(0.1f, rgb2, has2));
    std::printf("n %d\n", n);
    for (int i = 0; i < n; ++i) std::printf("%d %d %d %d %d %d %d %d\n", rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], has[i],
                                            rgb2[3 * i], rgb2[3 * i + 1], rgb2[3 * i + 2], has2[i]);
    std::printf("coloured %lld\n", coloured);
    for (int i = 0; i < n; ++i) std::printf("xyz %.9g %.9g %.9g\n", x[i], y[i], z[i]);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
"""


def test_shim_smooth_colors_with_local_region(tmp_path):
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    src = tmp_path / "shim_local_smooth.cpp"
    src.write_text(_SHIM_PROGRAM)
    exe = tmp_path / "shim_local_smooth"
    cmd = ["g++", "-std=c++17", "-O2", "-I", _build.INCLUDE, "-I", host_build.HOST, str(src), "-L", _build.LIB_DIR, "-lpcp_hip",
           "-Wl,-rpath," + _build.LIB_DIR, "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    n = int(lines[0].split()[1])
    vals = np.array([[int(v) for v in l.split()] for l in lines[1:1 + n]], np.int64)
    coloured = int(lines[1 + n].split()[1])
    xyz = np.array([[np.float32(float(v)) for v in l.split()[1:]] for l in lines[2 + n:2 + 2 * n]], np.float32)
    words = (vals[:, 0] | (vals[:, 1] << 8) | (vals[:, 2] << 16) | (vals[:, 3] << 24)).astype(np.uint32)
    want = ref.smooth_local(xyz[:, 0], xyz[:, 1], xyz[:, 2], words, 0.1)
    r, g, b = ref.split(want)
    assert np.array_equal(vals[:, 4:7], np.stack([r, g, b], 1))
    assert np.array_equal(vals[:, 7], (want >> 24) & 1)
    assert coloured == int(((want >> 24) & 1).sum())
    assert vals[:, 3].sum() > 100
