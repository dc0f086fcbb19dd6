"""The orthographic maps above the C ABI ("Orthographic maps"): pipeline.PointCloudColorizer.ortho_map after run(),
and pipeline.CloudSmooth.process_and_colourise_streamed(..., ortho=...) on the two-level MLS scene of test_stream_colour_gpu.py,
where the map is accumulated over the chunks.  The layers equal the restatement in _ortho_ref.py over the downloaded rows, and a
run with download=False -- where nothing but the map leaves the device -- returns the same bytes."""
import numpy as np
import pytest

import _ortho_ref as ref
from conftest import cam_struct
from test_stream_colour_gpu import CHUNK, _levels_scene, _mls_params, _views

pytestmark = pytest.mark.gpu


def test_ortho_map_after_run(small_scene):
    from pointcloudprocessor_amd import capi, pipeline

    s = small_scene
    eng = pipeline.HipEngine(0)
    try:
        eng.configure(cam_struct(capi, s["cam"]))
        eng.upload_cloud(s["x"], s["y"], s["z"])
        eng.set_keyframes(s["poses"], s["images"], s["masks"])
        col = pipeline.PointCloudColorizer(eng)
        out = col.run(fuse_labels=True)
        xyz = np.stack([s["x"], s["y"], s["z"]], axis=1)
        mean_pose = np.asarray(s["poses"], np.float64).reshape(-1, 7)[:, :3].mean(axis=0)
        with pytest.raises(ValueError, match="xyz"):
            col.ortho_map("auto", gsd=0.05)  # nothing of the upload is kept: the map to fit is the caller's to pass
        with pytest.raises(ValueError, match="rows"):
            col.ortho_map("auto", gsd=0.05, xyz=xyz[:-1])
        for frame in (ref.down_frame(0.05), "auto"):
            got = col.ortho_map(frame, gsd=0.05, fill_radius=2, xyz=(s["x"], s["y"], s["z"]), viewer=mean_pose)
            fr = got["frame"]
            want = ref.ortho(fr, xyz, out["rgb"], label=out["label"], has=out["has"], fill_radius=2)
            assert ref.same(got, want, with_label=True) is None, f"{ref.same(got, want, True)} differs"
            assert (got["contributors"], got["occupied"], got["filled"]) == (want["contributors"], want["occupied"], want["filled"])
            assert want["occupied"] >= 300
        assert got["contributors"] == int(out["has"].sum()), "every coloured row lies inside the fitted frame"
        # the fitted frame is the library's fit of the coloured rows, and looks at them from the keyframes' side
        assert fr == capi.ortho_fit_frame_host(xyz, 0.05, has=out["has"], viewer=mean_pose).as_dict()
        assert np.dot(mean_pose - np.array(fr["o"]), np.array(fr["n"])) < 0
        other = col.ortho_map("auto", gsd=0.05, xyz=xyz, viewer=np.array(fr["o"]) + 20 * np.array(fr["n"]))["frame"]
        assert np.allclose(other["n"], -np.array(fr["n"]), atol=1e-6), "a viewer on the other side turns n round"
        # the crack layers are the map's arrays at the index layer
        n = len(xyz)
        fake = dict(width_mean=np.arange(n, dtype=np.float32) + 1, label=np.arange(n, dtype=np.int32))
        layered = col.ortho_map(fr, fill_radius=2, crack_map=fake)
        empty = layered["index"] == 0xFFFFFFFF
        assert (layered["crack"][empty] == -1).all() and (layered["width"][empty] == 0).all() and empty.any() and not empty.all()
        assert (layered["crack"][~empty] == layered["index"][~empty].astype(np.int32)).all()
        assert (layered["width"][~empty] == layered["index"][~empty].astype(np.float32) + 1).all()
        assert "width" not in got and "crack" not in got, "no crack map exists: no crack layers"
        with pytest.raises(capi.PcpError) as e:
            eng.ctx.ortho_stats()  # the map ended with the call
        assert e.value.code == capi.PCP_ERR_STATE
        with pytest.raises(ValueError, match="ortho_map.*index shard"):
            pipeline.PointCloudColorizer(eng, rank=0, world=2).ortho_map(fr)
    finally:
        eng.close()


@pytest.mark.parametrize("fuse", [False, True])
def test_streamed_map_equals_the_restatement_and_the_run_without_download(fuse):
    from pointcloudprocessor_amd import capi, pipeline

    s = _levels_scene()
    smooth, colour = pipeline.HipEngine(0), pipeline.HipEngine(0)
    try:
        _views(colour.ctx, capi, s, masks=fuse)
        cs = pipeline.CloudSmooth(smooth, _mls_params(capi))
        smooth.upload_cloud(s["x"], s["y"], s["z"])
        raw = np.stack([s["x"], s["y"], s["z"]], axis=1)
        # a bad frame is refused before the chain starts: no sweep has run, no stream is open
        with pytest.raises(capi.PcpError) as e:
            next(cs.process_and_colourise_streamed(colour, CHUNK, ortho=dict(
                frame=ref.frame((1.6, -1.2, 0.0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 0.004, 16385, 100, 0.0, 10.0))))
        assert e.value.code == capi.PCP_ERR_RANGE and not hasattr(cs, "streamed_colour")
        with pytest.raises(ValueError, match="xyz"):
            next(cs.process_and_colourise_streamed(colour, CHUNK, ortho=dict(frame="auto", gsd=0.004)))
        # the keyframes look along +z at the two patches (x 1.70..2.35, y -1.1..-0.9, z 1.5 and 1.9): 4 mm pixels
        ortho = dict(frame=ref.frame((1.6, -1.2, 0.0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 0.004, 220, 100, 0.0, 10.0), fill_radius=2)
        parts = list(cs.process_and_colourise_streamed(colour, CHUNK, fuse_labels=fuse, ortho=ortho))
        st, got = cs.streamed_colour, cs.ortho_output
        print("streamed ortho map:", {k: v for k, v in st.items()}, got["frame"])
        assert st["chunks"] >= 3 and len(parts) >= 3 and st["ortho"]["adds"] >= 3
        cat = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        assert ("label" in got) == fuse
        # Every row of this scene takes a colour, so a row's place in the concatenated chunks IS its global index (the rows of
        # the chunks before it plus its row in its own chunk): the index layer is compared exactly, like every other layer.
        assert st["coloured"] == st["rows"] == len(cat["xyz"]), "every smoothed row is coloured"
        want = ref.ortho(got["frame"], cat["xyz"], cat["rgb"], label=cat["label"] if fuse else None, fill_radius=2)
        assert ref.same(got, want, with_label=fuse) is None, f"{ref.same(got, want, fuse)} differs"
        first_rows = len(parts[0]["xyz"])
        assert (got["index"][want["status"] == 1] >= first_rows).sum() >= 1000, "pixels won by rows of later chunks"
        assert (got["occupied"], got["filled"]) == (want["occupied"], want["filled"]) and want["occupied"] >= 1000 and want["filled"] >= 100
        assert st["ortho"]["contributors"] == st["coloured"] == len(cat["xyz"]), "the frame holds every coloured row"
        # the map ended with the generator
        with pytest.raises(capi.PcpError) as e:
            colour.ctx.ortho_stats()
        assert e.value.code == capi.PCP_ERR_STATE
        # the configuration the feature is for: the chunks' rows stay on the device
        smooth.upload_cloud(s["x"], s["y"], s["z"])
        counts = list(cs.process_and_colourise_streamed(colour, CHUNK, fuse_labels=fuse, download=False, ortho=ortho))
        assert all(set(p) == {"count"} for p in counts) and [p["count"] for p in counts] == [len(p["xyz"]) for p in parts]
        assert ref.same(cs.ortho_output, got, with_label=fuse) is None
        # "auto": the plane fitted on the host to the raw map, seen from the side of the viewer -- here the mean keyframe
        # position, and a point on the other side of the plane, which turns n round
        viewer = np.asarray(s["poses"], np.float64)[:, :3].mean(axis=0)
        frames = []
        for v in (viewer, None, 2 * raw.mean(axis=0).astype(np.float64) - viewer):
            smooth.upload_cloud(s["x"], s["y"], s["z"])
            list(cs.process_and_colourise_streamed(colour, CHUNK, fuse_labels=fuse, download=False,
                                                   ortho=dict(frame="auto", gsd=0.004, xyz=(s["x"], s["y"], s["z"]), viewer=v)))
            assert cs.ortho_output["frame"] == capi.ortho_fit_frame_host(raw, 0.004, viewer=v).as_dict()
            assert 0 < cs.ortho_output["occupied"] <= cs.ortho_output["contributors"]
            frames.append(cs.ortho_output["frame"])
        assert np.dot(viewer - np.array(frames[0]["o"]), np.array(frames[0]["n"])) < 0
        assert np.allclose(frames[2]["n"], -np.array(frames[0]["n"]), atol=1e-6)
        # off: no map, the chunks as before
        smooth.upload_cloud(s["x"], s["y"], s["z"])
        plain = list(cs.process_and_colourise_streamed(colour, CHUNK, fuse_labels=fuse))
        assert cs.ortho_output is None and "ortho" not in cs.streamed_colour
        for a, b in zip(plain, parts):
            assert all(a[k].tobytes() == b[k].tobytes() for k in b)
    finally:
        smooth.close()
        colour.close()
