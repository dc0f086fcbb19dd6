"""pipeline.CloudSmooth.process_and_colourise_streamed(..., output_leaf=...): the voxel-grid output ("Voxel-grid
output") accumulated over the chunks of the streamed chain, on the two-level MLS scene of test_stream_colour_gpu.py.  The
reduced rows equal the restatement over the concatenated downloaded chunks, and a run with download=False -- where nothing
but the reduced rows leaves the device -- returns the same bytes."""
import numpy as np
import pytest

import _voxel_reduce_ref as ref
from test_stream_colour_gpu import CHUNK, _levels_scene, _mls_params, _views

pytestmark = pytest.mark.gpu

LEAF = 0.01  # the scene's smoothed rows lie about 3 mm apart: most voxels hold several rows, from one chunk or two


@pytest.mark.parametrize("fuse", [False, True])
def test_streamed_voxel_output_equals_the_restatement_and_the_run_without_download(fuse):
    from pointcloudprocessor_amd import capi, pipeline

    s = _levels_scene()
    smooth, colour = pipeline.HipEngine(0), pipeline.HipEngine(0)
    try:
        _views(colour.ctx, capi, s, masks=fuse)
        cs = pipeline.CloudSmooth(smooth, _mls_params(capi))
        smooth.ctx.upload_cloud(s["x"], s["y"], s["z"])
        parts = list(cs.process_and_colourise_streamed(colour, CHUNK, fuse_labels=fuse, output_leaf=LEAF))
        st, got = cs.streamed_colour, cs.voxel_output
        print("streamed voxel output:", {k: v for k, v in st.items() if k != "voxel_add_chunk_s"})
        assert st["chunks"] >= 3 and len(parts) >= 3
        cat = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        assert ("label" in cat) == fuse and ("label" in got) == fuse
        want = ref.reduce(LEAF, cat["xyz"], cat["rgb"], cat["label"] if fuse else None)
        assert ref.same(got, want, fuse) is None, f"{ref.same(got, want, fuse)} differs"
        vox = st["voxel"]
        assert vox["rows"] == st["coloured"] == len(cat["index"]) and vox["voxels"] == len(want["count"]) == len(got["count"])
        assert 2 * len(want["count"]) < len(cat["index"]), "the leaf merges rows"
        assert len(st["voxel_add_chunk_s"]) == len(parts) and st["voxel_finish_s"] > 0.0
        # the accumulation ended with the generator
        with pytest.raises(capi.PcpError) as e:
            colour.ctx.voxel_reduce_stats()
        assert e.value.code == capi.PCP_ERR_STATE
        # the configuration the feature is for: the chunks' rows stay on the device
        smooth.ctx.upload_cloud(s["x"], s["y"], s["z"])
        counts = list(cs.process_and_colourise_streamed(colour, CHUNK, fuse_labels=fuse, download=False, output_leaf=LEAF))
        assert all(set(p) == {"count"} for p in counts) and [p["count"] for p in counts] == [len(p["index"]) for p in parts]
        assert ref.same(cs.voxel_output, got, fuse) is None
        assert cs.streamed_colour["voxel"]["rows"] == vox["rows"]
        # off: no accumulation, no voxel output, the chunks as before
        smooth.ctx.upload_cloud(s["x"], s["y"], s["z"])
        plain = list(cs.process_and_colourise_streamed(colour, CHUNK, fuse_labels=fuse))
        assert cs.voxel_output is None and "voxel" not in cs.streamed_colour
        for a, b in zip(plain, parts):
            assert all(a[k].tobytes() == b[k].tobytes() for k in b)
    finally:
        smooth.close()
        colour.close()
