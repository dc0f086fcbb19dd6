"""The orthophoto above the C ABI ("Orthophotos"): pipeline.PointCloudColorizer.ortho_map(texture=...) after run(),
and pipeline.CloudSmooth.process_and_colourise_streamed(..., ortho=dict(..., texture=...)) on the two-level MLS scene of
test_stream_colour_gpu.py, where the photo is textured after the last chunk on the merged depth maps.  Every layer and count
equals the restatement in _ortho_texture_ref.py -- in the streamed form over the concatenated rows, whose depth maps are the
merged ones -- and a run with download=False returns the same bytes."""
import numpy as np
import pytest

import _ortho_ref as oref
import _ortho_texture_ref as ref
from conftest import cam_struct
from test_stream_colour_gpu import CHUNK, _levels_scene, _mls_params, _views

pytestmark = pytest.mark.gpu


def _same(got, want):
    bad = ref.same(got, want)
    assert bad is None, f"{bad} differs"


def test_ortho_map_with_a_texture_after_run(small_scene):
    from pointcloudprocessor_amd import capi, pipeline

    s = small_scene
    eng = pipeline.HipEngine(0)
    try:
        eng.configure(cam_struct(capi, s["cam"]))
        eng.upload_cloud(s["x"], s["y"], s["z"])
        eng.set_keyframes(s["poses"], s["images"], s["masks"])
        col = pipeline.PointCloudColorizer(eng)
        col.run()
        fr = oref.down_frame(0.05)
        plain = col.ortho_map(fr, fill_radius=2)
        assert "photo" not in plain
        w2cs, dmaps = ref.depth_maps(s["cam"], s["poses"], s["x"], s["y"], s["z"])
        for texture in (dict(scale=4, views=5, interpolate=False), dict(scale=3), dict(scale=2, views=3, max_step=0.01)):
            got = col.ortho_map(fr, fill_radius=2, texture=texture)
            for key in oref.LAYERS:  # the map's own layers are what they are without the texture
                assert got[key].tobytes() == plain[key].tobytes(), key
            want = ref.texture(s["cam"], s["poses"], s["images"], s["masks"], w2cs, dmaps, fr, got["source"], got["depth"], texture["scale"],
                               texture.get("views", 1), texture.get("interpolate", True), texture.get("max_step", 0.05))
            assert want["textured"] >= 2500 * texture["scale"] ** 2 and want["unseen"] > 0
            _same(got["photo"], want)
            assert got["photo"]["skipped_pairs"] > 0
        for bad in (dict(views=5), dict(scale=4, sharp=True)):
            with pytest.raises(ValueError, match="texture"):
                col.ortho_map(fr, texture=bad)
        with pytest.raises(capi.PcpError) as e:
            col.ortho_map(fr, texture=dict(scale=17))
        assert e.value.code == capi.PCP_ERR_INVALID
        with pytest.raises(capi.PcpError) as e:
            eng.ctx.ortho_stats()  # the map ended with the refused call too
        assert e.value.code == capi.PCP_ERR_STATE
        with pytest.raises(ValueError, match="ortho_map.*index shard"):
            pipeline.PointCloudColorizer(eng, rank=0, world=2).ortho_map(fr, texture=dict(scale=2))
    finally:
        eng.close()


def test_streamed_photo_equals_the_restatement_and_the_run_without_download():
    from pointcloudprocessor_amd import capi, pipeline

    s = _levels_scene()
    smooth, colour = pipeline.HipEngine(0), pipeline.HipEngine(0)
    try:
        _views(colour.ctx, capi, s, masks=True)
        cs = pipeline.CloudSmooth(smooth, _mls_params(capi))
        smooth.upload_cloud(s["x"], s["y"], s["z"])
        # the keyframes look along +z at the two patches (x 1.70..2.35, y -1.1..-0.9, z 1.5 and 1.9): 4 mm pixels, 2 mm fine ones
        ortho = dict(frame=oref.frame((1.6, -1.2, 0.0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 0.004, 220, 100, 0.0, 10.0), fill_radius=2,
                     texture=dict(scale=2, views=5, interpolate=True, max_step=0.05))
        parts = list(cs.process_and_colourise_streamed(colour, CHUNK, ortho=ortho))
        st, got = cs.streamed_colour, cs.ortho_output
        assert st["chunks"] >= 3 and len(parts) >= 3 and "ortho_texture_s" in st
        cat = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        assert st["coloured"] == st["rows"] == len(cat["xyz"]), "every smoothed row is coloured: the chunks' rows are the whole cloud"
        # the depth maps of the concatenated rows ARE the merged ones
        w2cs, dmaps = ref.depth_maps(s["cam"], s["poses"], cat["xyz"][:, 0], cat["xyz"][:, 1], cat["xyz"][:, 2])
        want = ref.texture(s["cam"], s["poses"], s["images"], s["masks"], w2cs, dmaps, got["frame"], got["source"], got["depth"], 2, 5, True, 0.05)
        print({k: v for k, v in want.items() if not isinstance(v, np.ndarray)}, "views", np.unique(want["view"]))
        assert want["rgb"].shape == (200, 440, 3) and want["textured"] >= 10000 and want["two_or_more"] >= 5000
        assert want["refused_by_keep"] >= 1000, "the near patch hides part of the far one: only the merged maps say so"
        _same(got["photo"], want)
        # the last chunk's own maps would not do: the photo under them differs
        last = parts[-1]["xyz"]
        _, own = ref.depth_maps(s["cam"], s["poses"], last[:, 0], last[:, 1], last[:, 2])
        other = ref.texture(s["cam"], s["poses"], s["images"], s["masks"], w2cs, own, got["frame"], got["source"], got["depth"], 2, 5, True, 0.05)
        assert ref.same(other, want) is not None
        # the configuration the feature is for: the chunks' rows stay on the device
        smooth.upload_cloud(s["x"], s["y"], s["z"])
        counts = list(cs.process_and_colourise_streamed(colour, CHUNK, download=False, ortho=ortho))
        assert all(set(p) == {"count"} for p in counts)
        assert oref.same(cs.ortho_output, got) is None
        _same(cs.ortho_output["photo"], got["photo"])
        assert cs.ortho_output["photo"]["skipped_pairs"] == got["photo"]["skipped_pairs"]
        # without the texture: no photo, the same map
        smooth.upload_cloud(s["x"], s["y"], s["z"])
        list(cs.process_and_colourise_streamed(colour, CHUNK, download=False, ortho={k: v for k, v in ortho.items() if k != "texture"}))
        assert "photo" not in cs.ortho_output and oref.same(cs.ortho_output, got) is None and "ortho_texture_s" not in cs.streamed_colour
        # a bad request is refused before the chain starts
        with pytest.raises(ValueError, match="texture"):
            next(cs.process_and_colourise_streamed(colour, CHUNK, ortho=dict(ortho, texture=dict(views=2))))
    finally:
        smooth.close()
        colour.close()
