"""Fused segmentation labels at BASELINE.json's full single-GPU size (10 M points x 256 keyframes @1920x1080, with masks):
label, hits and views of EVERY point against the expectation derived from the oracle's top lists (OpenMP on the host cores),
bit for bit, and the colours against a fusion-off run of the same context."""
import numpy as np
import pytest

import _label_fusion_ref as lf
from conftest import cam_struct

pytestmark = pytest.mark.gpu

N, F = 10_000_000, 256


def test_full_size_labels_equal_the_oracle_expectation(oracle):
    from pointcloudprocessor_amd import capi, synth

    cd = synth.camera_dict("cfg")
    W, H = cd["image_width"], cd["image_height"]
    x, y, z, _ = synth.make_cloud(N)
    poses, _ = synth.make_trajectory(F)
    images = [synth.make_image(f, W, H) for f in range(F)]
    masks = []
    for f in range(F):  # gray masks with the discs at 255: every label value occurs
        g = images[(f + 100) % F][:, :, 0].copy()
        g[synth.make_mask(f, W, H) == 255] = 255
        masks.append(g)
    ctx = capi.Context(0)
    cull = capi.default_cull_params()
    ctx.set_camera(cam_struct(capi, cd), cull)
    ctx.upload_cloud(x, y, z)
    ctx.set_frames(poses)
    for f in range(F):
        ctx.upload_image(f, images[f])
        ctx.upload_mask(f, masks[f])
    off = ctx.colorize()
    ctx.set_label_fusion(True)
    on = ctx.colorize()
    lab = ctx.colour_labels()
    ctx.close()
    assert np.array_equal(off["rgb"], on["rgb"]) and np.array_equal(off["has"], on["has"])
    ocam, ocp = cam_struct(oracle, cd), oracle.default_cull_params()
    ocp.match_mode = cull.match_mode
    e = lf.expected(oracle, ocam, ocp, x, y, z, poses, images, masks, threads=oracle.hardware_threads())
    assert np.array_equal(on["has"] > 0, e["has"] > 0) and np.array_equal(on["rgb"], e["rgb"])
    assert (e["views"] > 0).sum() > 0.3 * N and (e["count"] > 5).sum() > 0.1 * N
    assert ((e["label"] > 0) & (e["label"] < 255)).sum() > 0.2 * N
    assert ((e["hits"] > 0) & (e["hits"] < e["views"])).sum() > 0.01 * N
    for k in ("label", "hits", "views"):
        bad = int((lab[k] != e[k]).sum())
        assert bad == 0, (k, bad)
