"""The keyframe colour balance on the GPU ("Image balance"): Context.image_balance against the host form stage by
stage (histograms, tables, pixels), and the upload property through the three upload paths: a keyframe uploaded with balance on
has, bit for bit, the texels of a plain upload of image_balance_host's output, with the same set_image_adjust setting and the
mask byte untouched.  Every comparison is exact equality."""
import subprocess

import numpy as np
import pytest
import torch

import _image_balance_ref as ref
from conftest import cam_struct

PIL = pytest.importorskip("PIL.Image")

pytestmark = pytest.mark.gpu

ADJUSTS = [None, (1.0, 1.0), (1.2, 0.9)]


def _context(w, h, n_frames):
    from pointcloudprocessor_amd import capi, synth

    ctx = capi.Context(0)
    cd = synth.camera_dict("tiny")
    cd.update(image_width=w, image_height=h)
    ctx.set_camera(capi.camera_from_dict(cd))
    x, y, z, _ = synth.make_cloud(2000)
    poses, _ = synth.make_trajectory(n_frames)
    ctx.upload_cloud(x, y, z)
    ctx.set_frames(poses)
    return ctx


def _param_sets():
    """every clip limit with both stages (the gammas in turn), then each stage alone"""
    sets = [dict(stages=3, clip_limit=c, gamma=ref.GAMMAS[k % 3]) for k, c in enumerate(ref.CLIPS)]
    return sets + [dict(stages=1, clip_limit=3.0, gamma=0.8), dict(stages=2, clip_limit=1.0, gamma=1.1)]


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocessor_amd import capi

    with capi.Context(0) as c:
        yield c


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_t{s[2]}x{s[3]}")
def test_device_form_equals_host_form_stage_by_stage(ctx, shape):
    from pointcloudprocessor_amd import capi

    w, h, tx, ty = shape
    for kind in ref.IMAGES:
        im = ref.image(kind, w, h)
        for ps in _param_sets():
            p = dict(ps, tiles=(tx, ty))
            want = capi.image_balance_host(im, p, stages=True)
            got = ctx.image_balance(im, p, stages=True)
            for key in ("hist", "lut", "bgr"):
                if key in want:
                    assert np.array_equal(got[key], want[key]), (kind, ps, key, int((got[key] != want[key]).sum()))
                else:
                    assert key not in got
            if ps["stages"] == 3 and kind == "noise":
                assert (want["bgr"] != im).mean() > 0.5, "the stage changes the picture"


def test_device_form_at_1080p_with_the_defaults(ctx):
    from pointcloudprocessor_amd import capi

    im = ref.looks_real(1920, 1080)
    want = capi.image_balance_host(im, True, stages=True)
    got = ctx.image_balance(im, True, stages=True)
    for key in ("hist", "lut", "bgr"):
        assert np.array_equal(got[key], want[key]), key
    # a view with a row stride: the same pixels
    wide = np.zeros((1080, 1920 + 5, 3), np.uint8)
    wide[:, :1920] = im
    assert np.array_equal(ctx.image_balance(wide[:, :1920], True), want["bgr"])


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["image_dump"]


def _jpeg(tmp_path, im, name):
    """(coefficient blob, the host decoder's pixels) of im saved as a JPEG"""
    p = tmp_path / f"{name}.jpg"
    PIL.fromarray(np.ascontiguousarray(im[:, :, ::-1])).save(p, quality=92, subsampling=2)
    r = subprocess.run([_exe(), str(p), str(p) + ".blob", "coeffs"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([_exe(), str(p), str(p) + ".raw"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head, _, body = open(str(p) + ".raw", "rb").read().partition(b"\n")
    w, h, c = map(int, head.split())
    return np.fromfile(str(p) + ".blob", np.uint8), np.frombuffer(body, np.uint8).reshape(h, w, c)


def _adjust(c, adjust):
    if adjust is None:
        c.set_image_adjust(False)
    else:
        c.set_image_adjust(True, *adjust)


@pytest.mark.parametrize("size", [(64, 48), (70, 50), (1920, 1080)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("path", ["image", "block", "jpeg"])
def test_upload_property(tmp_path, path, size):
    """balance on + raw frames == balance off + image_balance_host's frames, for each adjust setting"""
    from pointcloudprocessor_amd import capi

    w, h = size
    raw = ref.looks_real(w, h) if w > 100 else ref.image("noise", w, h, seed=3)
    blob = None
    if path == "jpeg":
        blob, raw = _jpeg(tmp_path, raw, f"k{w}")
    params = dict(stages=3, tiles=(8, 8), clip_limit=3.0, gamma=1.1)
    balanced = capi.image_balance_host(raw, params)
    assert (balanced != raw).mean() > 0.3
    pinned = torch.empty((2, h, w, 3), dtype=torch.uint8).pin_memory()
    stage = pinned.numpy()
    mask = (np.random.default_rng(5).random((h, w)) < 0.5).astype(np.uint8) * 255
    with _context(w, h, 3) as on, _context(w, h, 3) as off:
        on.set_image_balance(params)
        on.upload_mask(0, mask)
        off.upload_mask(0, mask)
        for f, adjust in enumerate(ADJUSTS):
            _adjust(on, adjust)
            _adjust(off, adjust)
            if path == "image":
                on.upload_image(f, raw)
                off.upload_image(f, balanced)
            elif path == "jpeg":
                on.upload_image_jpeg(f, blob)
                off.upload_image(f, balanced)
            else:
                stage[0] = raw
                on.upload_images_block(f, stage[:1])
                on.synchronize()
                stage[1] = balanced
                off.upload_images_block(f, stage[1:])
                off.synchronize()
            got, gmask = on.download_image(f)
            want, wmask = off.download_image(f)
            assert np.array_equal(got, want), (path, size, adjust, int((got != want).any(axis=2).sum()))
            assert np.array_equal(gmask, wmask) and np.array_equal(gmask, mask if f == 0 else np.zeros_like(mask))
            if adjust is None:
                assert np.array_equal(got, balanced)


def test_mask_before_and_after_the_image_survives():
    w, h = 70, 50
    raw = ref.image("blob", w, h)
    rng = np.random.default_rng(8)
    m0, m1 = (rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2))
    from pointcloudprocessor_amd import capi

    want = capi.image_balance_host(raw, True)
    with _context(w, h, 2) as c:
        c.set_image_balance(True)
        c.upload_mask(0, m0)
        c.upload_image(0, raw)
        c.upload_image(1, raw)
        c.upload_mask(1, m1)
        for f, m in ((0, m0), (1, m1)):
            got, mask = c.download_image(f)
            assert np.array_equal(mask, m) and np.array_equal(got, want)
        c.upload_image(1, raw)  # and again over a mask that is already there
        got, mask = c.download_image(1)
        assert np.array_equal(mask, m1) and np.array_equal(got, want)


def test_four_async_uploads_keep_their_own_scratch():
    """both lanes busy, one synchronise: a scratch buffer shared between lanes would mix the keyframes' tables"""
    from pointcloudprocessor_amd import capi

    w, h = 512, 384
    kinds = ["noise", "ramp", "blob", "two_level"]
    pinned = torch.empty((4, h, w, 3), dtype=torch.uint8).pin_memory()
    frames = pinned.numpy()
    for k, kind in enumerate(kinds):
        frames[k] = ref.image(kind, w, h, seed=k)
    params = dict(stages=3, tiles=(2, 2), clip_limit=3.0, gamma=0.8)
    with _context(w, h, 4) as c:
        c.set_image_balance(params)
        for k in range(4):
            c.upload_image_async(k, frames[k])
        c.synchronize()
        for k in range(4):
            got, _ = c.download_image(k)
            assert np.array_equal(got, capi.image_balance_host(frames[k], params)), kinds[k]


def test_reupload_with_other_parameters_and_off_again():
    from pointcloudprocessor_amd import capi

    w, h = 90, 60
    raw = ref.image("noise", w, h, seed=9)
    with _context(w, h, 1) as c:
        for params in (dict(stages=3, tiles=(3, 5), clip_limit=1.0, gamma=0.8), dict(stages=3, tiles=(8, 8), clip_limit=40.0, gamma=1.1),
                       dict(stages=2, gamma=0.8), dict(stages=1, tiles=(1, 1), clip_limit=0.0)):
            c.set_image_balance(params)
            c.upload_image(0, raw)
            assert np.array_equal(c.download_image(0)[0], capi.image_balance_host(raw, params)), params
        c.set_image_balance(None)
        c.upload_image(0, raw)
        assert np.array_equal(c.download_image(0)[0], raw)
        # a grid that cannot be reflected over the camera's image is refused at the upload, and nothing is touched
        c.set_image_balance(dict(tiles=(16, 16)))
        with _context(20, 8, 1) as small:
            small.set_image_balance(dict(tiles=(16, 16)))
            with pytest.raises(capi.PcpError) as e:
                small.upload_image(0, np.zeros((8, 20, 3), np.uint8))
            assert e.value.code == capi.PCP_ERR_RANGE
        with pytest.raises(capi.PcpError) as e:
            c.set_image_balance(dict(tiles=(17, 8)))
        assert e.value.code == capi.PCP_ERR_INVALID
        c.upload_image(0, raw)  # the refused setting changed nothing: 16 x 16 still holds
        assert np.array_equal(c.download_image(0)[0], capi.image_balance_host(raw, dict(tiles=(16, 16))))


def test_colours_end_to_end(gpu_ctx_factory, small_scene):
    """colorize with balance on == colorize of pre-balanced images with balance off, through HipEngine's balance= argument"""
    from pointcloudprocessor_amd import capi
    from pointcloudprocessor_amd.pipeline import HipEngine

    s = small_scene
    out = []
    for images, balance in ((s["images"], True), ([capi.image_balance_host(im, True) for im in s["images"]], None)):
        eng = HipEngine(0)
        try:
            eng.configure(cam_struct(capi, s["cam"]))
            eng.upload_cloud(s["x"], s["y"], s["z"])
            eng.set_keyframes(s["poses"], images=images, balance=balance)
            out.append(eng.ctx.colorize())
        finally:
            eng.close()
    assert np.array_equal(out[0]["rgb"], out[1]["rgb"]) and np.array_equal(out[0]["has"], out[1]["has"])
    assert out[0]["has"].sum() > 1000
    ctx = gpu_ctx_factory()
    ctx.set_camera(cam_struct(capi, s["cam"]))
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
    plain = ctx.colorize()
    assert (plain["rgb"] != out[0]["rgb"]).any(axis=1).sum() > 100, "skipping the stage would have been visible"
