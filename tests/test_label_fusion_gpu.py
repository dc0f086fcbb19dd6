"""Fused segmentation labels on the device (pcp_set_label_fusion / pcp_colour_labels): label, hits and views of every point,
bit for bit, against an expectation derived from the ORACLE (its top lists, its projection for each listed view's pixel,
the uploaded masks; tests/_label_fusion_ref.py does the exact-integer fusion) -- over every path, camera form, cull mode and
match mode of the colour stage, index shards, and the state rules of the new entry points.  In every case the colours and
`has` of the fusion-on run equal those of a fusion-off run."""
import numpy as np
import pytest

import _label_fusion_ref as lf
from conftest import cam_struct

pytestmark = pytest.mark.gpu

N_BIG, F_BIG = 60_000, 24


def _gray_mask(f, W, H):
    from pointcloudprocessor_amd import synth

    g = synth.make_image(f + 100, W, H)[:, :, 0].copy()
    g[synth.make_mask(f, W, H) == 255] = 255
    return g


_SCENES = {}


def _scene(kind, small_scene=None):
    """small: the suite's 20 k x 6 scene; disc / gray: 60 k points x 24 keyframes on the tiny camera with synth's disc masks
    / gray masks (a channel of another image, the discs at 255)"""
    from pointcloudprocessor_amd import synth

    if kind == "small":
        s = small_scene
        return dict(cam=s["cam"], x=s["x"], y=s["y"], z=s["z"], poses=s["poses"], images=s["images"], masks=s["masks"])
    if kind not in _SCENES:
        cd = synth.camera_dict("tiny")
        W, H = cd["image_width"], cd["image_height"]
        x, y, z, _ = synth.make_cloud(N_BIG)
        poses, _ = synth.make_trajectory(F_BIG)
        images = [synth.make_image(f, W, H) for f in range(F_BIG)]
        masks = [synth.make_mask(f, W, H) if kind == "disc" else _gray_mask(f, W, H) for f in range(F_BIG)]
        _SCENES[kind] = dict(cam=cd, x=x, y=y, z=z, poses=poses, images=images, masks=masks)
    return _SCENES[kind]


def _cull(module, cull_mode=0, match_mode=1, zbuf=1):
    cp = module.default_cull_params()
    cp.cull_mode, cp.match_mode, cp.enable_depth_buffer_culling = cull_mode, match_mode, zbuf
    return cp


def _load(ctx, capi, s, cull, masks=True, lo=0, hi=None):
    ctx.set_camera(cam_struct(capi, s["cam"]), cull)
    ctx.upload_cloud(s["x"][lo:hi], s["y"][lo:hi], s["z"][lo:hi])
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
        if masks:
            ctx.upload_mask(f, s["masks"][f])


def _expect(oracle, s, cull_mode=0, match_mode=1, zbuf=1):
    """the oracle-side expectation; PCP_MATCH_RADIUS is the oracle's faithful mode (over its ROUNDTRIP arithmetic)"""
    from pointcloudprocessor_amd import capi

    radius = match_mode == capi.MATCH_RADIUS
    ocp = _cull(oracle, cull_mode, 1 if radius else match_mode, zbuf)
    return lf.expected(oracle, cam_struct(oracle, s["cam"]), ocp, s["x"], s["y"], s["z"], s["poses"], s["images"], s["masks"],
                       faithful=radius, threads=8)


def _same_labels(got, e, what=""):
    for k in ("label", "hits", "views"):
        bad = np.nonzero(got[k] != e[k])[0]
        assert not len(bad), (what, k, len(bad), bad[:5], got[k][bad[:5]], e[k][bad[:5]])


def _run(ctx, path):
    """one colour result by the named path; returns the colours"""
    if path == "colorize":
        return ctx.colorize()
    ctx.colour_reset()
    ctx.depth_pass()
    if path == "from_depth":
        return ctx.colorize_from_depth()
    F = ctx.n_frames
    a, b = F // 3, F - F // 4
    for f0, f1 in ((0, a), (a, b), (b, F)):
        ctx.colour_pass(f0, f1)
    r = ctx.colour_finalise(want_top=True)
    assert not (r["top_rgb"] >> 24).any(), "out_top_rgb is 0x00RRGGBB in both forms"
    return r


def _off_then_on(ctx, path):
    """(colours with fusion off, colours with fusion on, labels)"""
    ctx.colour_reset()
    ctx.set_label_fusion(False)
    off = _run(ctx, path)
    ctx.colour_reset()
    ctx.set_label_fusion(True)
    on = _run(ctx, path)
    lab = ctx.colour_labels()
    for k in ("rgb", "has") + (("count", "top_score", "top_rgb", "top_frame") if path == "ranges" else ()):
        assert np.array_equal(off[k], on[k]), (path, k)
    return off, on, lab


def _packed_words(ctx):
    import torch

    from pointcloudprocessor_amd import pipeline

    ptr, n = ctx.colour_labels_device()
    ctx.synchronize()
    return torch.as_tensor(pipeline._DeviceArray(ptr, n, "<i4"), device="cuda:0").cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", ["small", "disc", "gray"])
def test_labels_equal_the_oracle_expectation(gpu_ctx_factory, oracle, small_scene, kind):
    from pointcloudprocessor_amd import capi

    s = _scene(kind, small_scene)
    e = _expect(oracle, s)
    seen = e["views"] > 0
    assert seen.sum() > 500
    if kind == "gray":  # the cases that make the check mean something, counted on the oracle's side
        assert (e["count"] > 5).sum() >= 1000
        assert ((e["hits"] > 0) & (e["hits"] < e["views"])).sum() >= 800
        assert ((e["label"] > 0) & (e["label"] < 255)).sum() >= 5000
    ctx = gpu_ctx_factory()
    _load(ctx, capi, s, _cull(capi))
    for path in ("colorize", "from_depth", "ranges"):
        off, on, lab = _off_then_on(ctx, path)
        _same_labels(lab, e, path)
        assert np.array_equal(on["rgb"], e["rgb"]) and np.array_equal(on["has"], e["has"])
        # unseen points: the word 0; the packed device words are label | hits<<8 | views<<16
        w = _packed_words(ctx)
        assert len(w) == len(s["x"]) and not w[~seen].any()
        assert np.array_equal(w, lab["label"].astype(np.uint32) | (lab["hits"].astype(np.uint32) << 8)
                              | (lab["views"].astype(np.uint32) << 16))
    # nullable outputs
    import ctypes as C

    only = np.empty(len(s["x"]), np.uint8)
    assert ctx.lib.pcp_colour_labels(ctx.h, None, only.ctypes.data_as(C.c_void_p), None) == 0
    assert np.array_equal(only, e["hits"])
    assert ctx.lib.pcp_colour_labels(ctx.h, None, None, None) == 0
    ctx.close()


@pytest.mark.parametrize("path", ["colorize", "from_depth", "ranges"])
@pytest.mark.parametrize("cull_mode,zbuf", [(0, 1), (0, 0), (1, 0), (2, 1)])
@pytest.mark.parametrize("match_mode", [0, 1])
def test_every_cull_and_match_mode_on_every_path(gpu_ctx_factory, oracle, small_scene, path, cull_mode, zbuf, match_mode):
    """zbuf = 1 with PCP_CULL_ZBUFFER is the common camera form (its own kernel instantiations); the others take the general
    one; cull mode 2 reads hull bits."""
    from pointcloudprocessor_amd import capi

    s = _scene("small", small_scene)
    e = _expect(oracle, s, cull_mode, match_mode, zbuf)
    assert (e["views"] > 0).sum() > 300 and ((e["hits"] > 0) & (e["hits"] < e["views"])).sum() > 5
    ctx = gpu_ctx_factory()
    _load(ctx, capi, s, _cull(capi, cull_mode, match_mode, zbuf))
    off, on, lab = _off_then_on(ctx, path)
    _same_labels(lab, e, (path, cull_mode, zbuf, match_mode))
    assert np.array_equal(on["has"], e["has"]) and np.abs(on["rgb"].astype(int) - e["rgb"].astype(int)).max() <= 1
    ctx.close()


def _dup_scene(kind="gray"):
    """the 60 k x 24 scene with 3000 of its points copied exactly, multiplicity 2-4, the copies at other input indices"""
    s = dict(_scene(kind))
    rng = np.random.default_rng(17)
    n = len(s["x"])
    picks = rng.choice(n, 3000, replace=False)
    src = np.concatenate([np.arange(n)] + [picks[: 3000 // m] for m in (1, 2, 3)])
    order = rng.permutation(len(src))
    src = src[order]
    for k in "xyz":
        s[k] = np.ascontiguousarray(s[k][src])
    s["src"] = src
    return s


@pytest.mark.parametrize("cull_mode,zbuf", [(0, 1), (1, 0), (2, 1)])
@pytest.mark.parametrize("path", ["colorize", "ranges"])
def test_radius_match_on_exact_duplicates(gpu_ctx_factory, oracle, path, cull_mode, zbuf):
    """PCP_MATCH_RADIUS credits a point with its neighbours' samples, and with them the masks of the neighbours' pixels
    (k_match_fixup): on exact duplicates every copy's labels equal its twins' and the expectation from the oracle's
    faithful mode."""
    from pointcloudprocessor_amd import capi

    s = _dup_scene()
    e = _expect(oracle, s, cull_mode, capi.MATCH_RADIUS, zbuf)
    assert (e["count"] > np.minimum(e["count"], 5)).sum() > 1000
    ctx = gpu_ctx_factory()
    _load(ctx, capi, s, _cull(capi, cull_mode, capi.MATCH_RADIUS, zbuf))
    off, on, lab = _off_then_on(ctx, path)
    _same_labels(lab, e, (path, cull_mode))
    assert np.array_equal(on["rgb"], e["rgb"]) and np.array_equal(on["has"], e["has"])
    # twins: one value per source point
    src = s["src"]
    first = np.full(src.max() + 1, -1, np.int64)
    first[src[::-1]] = np.arange(len(src))[::-1]
    twins = np.nonzero(first[src] != np.arange(len(src)))[0]
    assert len(twins) >= 3000 and (lab["views"][twins] > 0).sum() > 100
    for k in ("label", "hits", "views"):
        assert np.array_equal(lab[k][twins], lab[k][first[src[twins]]]), k
    ctx.close()


@pytest.mark.parametrize("cull_mode", [0, 2])
def test_index_shards_concatenate_to_the_one_context_result(gpu_ctx_factory, oracle, cull_mode):
    """Two index shards (PCP_DEPTH_BATCHED) with MIN-merged depth maps -- in PCP_CULL_HPR, which has no depth maps, with the
    whole-map context's hull verdicts imported instead --: the shards' label arrays concatenate to the one-context result, which equals the expectation."""
    import torch

    from pointcloudprocessor_amd import capi, pipeline

    s = _scene("gray")
    n, F = len(s["x"]), len(s["poses"])
    cull = _cull(capi, cull_mode)
    e = _expect(oracle, s, cull_mode)

    def make(lo, hi, shard):
        eng = pipeline.HipEngine(0)
        if shard:
            eng.ctx.set_depth_source(True)
        _load(eng.ctx, capi, s, cull, lo=lo, hi=hi)
        eng.set_label_fusion(True)
        return eng

    full = make(0, n, False)
    col = pipeline.PointCloudColorizer(full).run(fuse_labels=True)
    _same_labels(col, e, "one context")
    assert np.array_equal(col["rgb"], e["rgb"])
    flags = [full.ctx.cull_frame(f)[0] for f in range(F)] if cull_mode == 2 else None
    engs, maps = [], []
    for r in range(2):
        lo, hi = pipeline.shard_bounds(n, r, 2)
        sh = make(lo, hi, True)
        sh.depth_pass()
        if flags is not None:
            for f in range(F):
                sh.ctx.hull_flags_import(f, flags[f][lo:hi])
        engs.append(sh)
        if flags is None:
            maps.append(sh.depth_maps_tensor())
    if maps:  # (the hull has no depth maps: its verdicts were imported above)
        merged = torch.minimum(maps[0], maps[1])
        for t in maps:
            t.copy_(merged)
        torch.cuda.synchronize()
    parts = []
    for sh in engs:
        c = sh.colour_from_depth()
        parts.append(dict(c, **sh.labels()))
    for k in ("label", "hits", "views", "rgb", "has"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), col[k]), k
    for eng in engs + [full]:
        eng.close()


def test_state_rules(gpu_ctx_factory, oracle, small_scene):
    from pointcloudprocessor_amd import capi

    s = _scene("small", small_scene)
    ctx = gpu_ctx_factory()
    # labels asked for with fusion off / before any result
    _load(ctx, capi, s, _cull(capi))
    ctx.colorize()
    for call in (ctx.colour_labels, ctx.colour_labels_device):
        with pytest.raises(capi.PcpError) as err:
            call()
        assert err.value.code == capi.PCP_ERR_STATE
    ctx.set_label_fusion(True)
    with pytest.raises(capi.PcpError) as err:  # the result at hand was produced with fusion off
        ctx.colour_labels()
    assert err.value.code == capi.PCP_ERR_STATE
    base = ctx.colorize()
    lab = ctx.colour_labels()
    e = _expect(oracle, s)
    _same_labels(lab, e)
    # the local colour smoothing changes the colours and leaves the labels alone
    ctx.colour_smooth_local(0.1)
    w = ctx.download_result_packed()
    assert not np.array_equal(w & 0xFF, base["rgb"][:, 0])
    _same_labels(ctx.colour_labels(), e, "after pcp_colour_smooth_local")
    # a later fusion-off result ends the labels
    ctx.set_label_fusion(False)
    _same_labels(ctx.colour_labels(), e, "switch off, same result")
    ctx.colorize()
    with pytest.raises(capi.PcpError) as err:
        ctx.colour_labels()
    assert err.value.code == capi.PCP_ERR_STATE
    # toggling while a top-5 accumulation is live
    ctx.colour_reset()
    ctx.depth_pass()
    ctx.colour_pass(0, 2)
    with pytest.raises(capi.PcpError) as err:
        ctx.set_label_fusion(True)
    assert err.value.code == capi.PCP_ERR_STATE
    ctx.set_label_fusion(False)  # no change: allowed
    ctx.colour_reset()
    ctx.set_label_fusion(True)
    ctx.colour_pass(0, 2)
    with pytest.raises(capi.PcpError) as err:
        ctx.set_label_fusion(False)
    assert err.value.code == capi.PCP_ERR_STATE
    ctx.colour_reset()
    # a keyframe without a mask: refused before anything runs, and it names the keyframe
    _load(ctx, capi, s, _cull(capi), masks=False)
    for f in (0, 1, 2, 4, 5):
        ctx.upload_mask(f, s["masks"][f])
    ctx.set_label_fusion(True)
    for call in (ctx.colorize, lambda: (ctx.depth_pass(), ctx.colorize_from_depth()), lambda: (ctx.depth_pass(), ctx.colour_pass(2, 5))):
        with pytest.raises(capi.PcpError) as err:
            call()
        assert err.value.code == capi.PCP_ERR_STATE and "keyframe 3" in str(err.value), str(err.value)
    ctx.colour_reset()
    ctx.depth_pass()
    ctx.colour_pass(0, 3)  # a range that has its masks
    ctx.colour_reset()
    ctx.set_label_fusion(False)
    ctx.colorize()  # and fusion off never asks for one
    ctx.close()


@pytest.mark.parametrize("n", [0, 1])
def test_degenerate_clouds(gpu_ctx_factory, oracle, small_scene, n):
    from pointcloudprocessor_amd import capi

    s = dict(_scene("small", small_scene))
    if n == 1:
        e_all = _expect(oracle, s)
        pick = int(np.argmax(e_all["views"] + (e_all["label"] > 0)))
        for k in "xyz":
            s[k] = s[k][pick:pick + 1].copy()
        e = _expect(oracle, s)  # alone, nothing occludes it
        assert e["views"][0] > 0
    else:
        for k in "xyz":
            s[k] = np.zeros(0, np.float32)
    ctx = gpu_ctx_factory()
    _load(ctx, capi, s, _cull(capi))
    ctx.set_label_fusion(True)
    for path in ("colorize", "from_depth", "ranges"):
        _run(ctx, path)
        lab = ctx.colour_labels()
        assert all(len(lab[k]) == n for k in lab)
        if n:
            _same_labels(lab, e, path)
        ptr, words = ctx.colour_labels_device()
        assert words == n
    # no keyframe processed: every point unseen
    ctx.colour_reset()
    r = ctx.colour_finalise()
    lab = ctx.colour_labels()
    assert not any(lab[k].any() for k in lab) and not r["has"].any()
    ctx.close()
