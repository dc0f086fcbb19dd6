"""The orthographic maps on the device ("Orthographic maps") against the restatement in _ortho_ref.py.  Every
comparison is exact equality.

The base scene is synth.make_cloud(20000) plus 300 exact copies of rows drawn with default_rng(7), added through
ortho_add_packed with every has bit set and hash colours, seen from above the room.  By the restatement: at gsd 0.05 a raster of
242 x 202 (four 64-row segments) with 11 556 occupied pixels, 3 144 of them with two or more contributors (up to 19), 173 ties
among the nearest, and a fill at R = 2 of 34 631 pixels that leaves 2 697 empty; at gsd 0.02 a raster of 602 x 502 (wider than
one 256-lane block) with 15 024 occupied pixels and a fill at R = 4 of 234 806 that leaves 52 374 empty; at gsd 0.2 a raster of
62 x 52 with up to 67 contributors per pixel.  The preconditions are asserted on the restatement's own counts."""
import numpy as np
import pytest

import _ortho_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

_BASE = {}


def _base(make):
    """the base scene uploaded once on a context of its own; the restatements by (gsd, R) are computed once and shared"""
    if not _BASE:
        s = ref.base_scene()
        for v in s.values():
            v.setflags(write=False)
        ctx = make()
        ctx.upload_cloud(s["xyz"][:, 0], s["xyz"][:, 1], s["xyz"][:, 2])
        _BASE.update(ctx=ctx, scene=s, want={})
    return _BASE


def _want(b, key, fr, radius, **kw):
    if key not in b["want"]:
        w = ref.ortho(fr, b["scene"]["xyz"], b["scene"]["rgb"], fill_radius=radius, **kw)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        b["want"][key] = w
    return b["want"][key]


def _map(ctx, fr, words, radius, index_base=0):
    ctx.ortho_begin(fr)
    added = ctx.ortho_add_packed(words, index_base)
    occupied, filled = ctx.ortho_finish(radius)
    return ctx.ortho_fetch(), added, occupied, filled


def _same(got, want, with_label=False):
    bad = ref.same(got, want, with_label)
    assert bad is None, f"{bad} differs"


@pytest.mark.parametrize("gsd", [0.05, 0.02, 0.2])
def test_device_equals_the_restatement(gpu_ctx_factory, gsd):
    b = _base(gpu_ctx_factory)
    ctx, s = b["ctx"], b["scene"]
    fr = ref.down_frame(gsd)
    for radius in (0, 2, 4):
        want = _want(b, (gsd, radius), fr, radius)
        pp = want["per_pixel"]
        empty = int((want["status"] == 0).sum())
        print(f"gsd {gsd} R {radius}: raster {fr['width']} x {fr['height']} occupied {want['occupied']} multi {(pp >= 2).sum()} "
              f"max {pp.max()} ties {want['ties']} filled {want['filled']} empty {empty}")
        if (gsd, radius) == (0.05, 2):
            assert (fr["width"], fr["height"]) == (242, 202)
            assert (pp >= 2).sum() >= 1000 and want["ties"] >= 50 and want["filled"] >= 1000 and empty >= 1000
        if (gsd, radius) == (0.02, 4):
            assert fr["width"] > 256 and fr["height"] > 256 and want["filled"] >= 1000 and empty >= 1000
        if gsd == 0.2:
            assert pp.max() >= 64, "a pixel with more contributors than a wavefront has lanes"
        got, added, occupied, filled = _map(ctx, fr, s["words"], radius)
        _same(got, want)
        assert (added, occupied, filled) == (want["contributors"], want["occupied"], want["filled"])
        st = ctx.ortho_stats()
        assert st == dict(contributors=added, atomics=st["atomics"], occupied=int((got["status"] == 1).sum()),
                          filled=int((got["status"] == 2).sum()), adds=1, pixels=fr["width"] * fr["height"])
        assert 0 < st["atomics"] <= added
        assert (got["source"][got["status"] == 1] == np.flatnonzero(got["status"].ravel() == 1)).all()
        # a second finish returns the same counts; another radius may follow on the same key image
        assert ctx.ortho_finish(radius) == (occupied, filled)
    assert ctx.ortho_finish(0) == (want["occupied"], 0)
    _same(ctx.ortho_fetch(), _want(b, (gsd, 0), fr, 0))
    ctx.ortho_end()


def test_a_refused_begin_keeps_the_live_map_and_its_shape(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi

    b = _base(gpu_ctx_factory)
    ctx, s = b["ctx"], b["scene"]
    fr = ref.down_frame(0.05)
    want = _want(b, (0.05, 2), fr, 2)
    got, _, _, _ = _map(ctx, fr, s["words"], 2)
    _same(got, want)
    # a smaller and a larger raster, each refused for another reason: the fetch after it is the live map's, 202 x 242
    for bad, code in ((dict(fr, width=10, height=10, n=[0.0, 0.0, 1.0]), capi.PCP_ERR_INVALID),
                      (dict(fr, width=500, height=400, gsd=2.0), capi.PCP_ERR_INVALID),
                      (dict(fr, width=16385, height=3), capi.PCP_ERR_RANGE)):
        with pytest.raises(capi.PcpError) as e:
            ctx.ortho_begin(bad)
        assert e.value.code == code
        again = ctx.ortho_fetch()
        assert again["index"].shape == (fr["height"], fr["width"])
        _same(again, want)
    ctx.ortho_end()


def test_depths_of_both_signs_and_a_window_that_cuts(gpu_ctx_factory):
    b = _base(gpu_ctx_factory)
    ctx, s = b["ctx"], b["scene"]
    inside = ref.down_frame(0.05, d_min=-100.0, d_max=100.0, oz=1.5)
    want = _want(b, "inside", inside, 1)
    direct = want["status"] == 1
    assert (want["depth"][direct] < 0).sum() >= 100 and (want["depth"][direct] > 0).sum() >= 100, "both signs win pixels"
    got, added, _, _ = _map(ctx, inside, s["words"], 1)
    _same(got, want)
    assert added == want["contributors"]
    cut = ref.down_frame(0.05, d_min=6.0)
    want = _want(b, "cut", cut, 0)
    assert 0 < want["contributors"] < len(s["xyz"]) and want["occupied"] < _want(b, (0.05, 0), ref.down_frame(0.05), 0)["occupied"]
    got, added, _, _ = _map(ctx, cut, s["words"], 0)
    _same(got, want)
    assert added == want["contributors"]
    # has bits: rows without one do not contribute
    has = np.random.default_rng(3).random(len(s["xyz"])) < 0.6
    words = np.where(has, s["words"], s["words"] & np.uint32(0x00FFFFFF)).astype(np.uint32)
    want = ref.ortho(ref.down_frame(0.05), s["xyz"], s["rgb"], has=has, fill_radius=2)
    got, added, _, _ = _map(ctx, ref.down_frame(0.05), words, 2)
    _same(got, want)
    assert added == want["contributors"] < int(has.sum()) + 1
    ctx.ortho_end()


def test_order_independence(gpu_ctx_factory):
    b = _base(gpu_ctx_factory)
    s = b["scene"]
    fr = ref.down_frame(0.05)
    want = _want(b, (0.05, 2), fr, 2)
    n = len(s["xyz"])
    ctx = gpu_ctx_factory()
    # the same rows under a permutation of the upload: row j of the upload is row perm[j] of the scene, so the winner of a
    # pixel is the restatement's on the permuted rows (ties go to the lowest index OF THE UPLOAD)
    perm = np.random.default_rng(21).permutation(n)
    xyz, rgb, words = s["xyz"][perm], s["rgb"][perm], s["words"][perm]
    ctx.upload_cloud(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    got, _, _, _ = _map(ctx, fr, words, 2)
    permuted = ref.ortho(fr, xyz, rgb, fill_radius=2)
    _same(got, permuted)
    for k in ("depth", "status", "source"):  # what does not name a row is the unpermuted map's
        assert got[k].tobytes() == want[k].tobytes(), k
    # the cloud added as two halves, in both orders: the one-shot's bytes
    half = n // 2
    parts = [(0, half), (half, n)]
    for order in (parts, parts[::-1]):
        ctx.ortho_begin(fr)
        added = 0
        for a, z in order:
            ctx.upload_cloud(s["xyz"][a:z, 0], s["xyz"][a:z, 1], s["xyz"][a:z, 2])
            added += ctx.ortho_add_packed(s["words"][a:z], index_base=a)
        assert ctx.ortho_finish(2) == (want["occupied"], want["filled"]) and added == want["contributors"]
        _same(ctx.ortho_fetch(), want)
        assert ctx.ortho_stats()["adds"] == 2
    # words in device memory of the context's GPU are taken as host words are
    import torch

    dev = torch.from_numpy(s["words"][half:n].view(np.int32).copy()).to("cuda:0")  # (the same 32 bits)
    torch.cuda.synchronize()
    ctx.ortho_begin(fr)
    ctx.upload_cloud(s["xyz"][half:, 0], s["xyz"][half:, 1], s["xyz"][half:, 2])
    ctx.ortho_add_packed(int(dev.data_ptr()), index_base=half)
    ctx.upload_cloud(s["xyz"][:half, 0], s["xyz"][:half, 1], s["xyz"][:half, 2])
    ctx.ortho_add_packed(s["words"][:half], index_base=0)
    ctx.ortho_finish(2)
    _same(ctx.ortho_fetch(), want)
    ctx.ortho_end()


def _views(ctx, capi, s):
    ctx.set_camera(cam_struct(capi, s["cam"]))
    e = np.zeros(0, np.float32)
    ctx.upload_cloud(e, e, e)
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
        ctx.upload_mask(f, s["masks"][f])


def test_colour_result_with_labels_and_the_state_rules(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    s = small_scene
    ctx = gpu_ctx_factory()
    _views(ctx, capi, s)
    ctx.set_label_fusion(True)
    ctx.upload_cloud(s["x"], s["y"], s["z"])
    fr = ref.down_frame(0.05)
    # state rules before anything is live
    for call in (lambda: ctx.ortho_add(0), lambda: ctx.ortho_finish(0), ctx.ortho_fetch, ctx.ortho_stats):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_STATE
    ctx.ortho_begin(fr)
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_add(0)  # no colour result yet
    assert e.value.code == capi.PCP_ERR_STATE
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_fetch()  # not finished
    assert e.value.code == capi.PCP_ERR_STATE
    ctx.colorize(download=False)
    rows = ctx.colour_compact(want_label=True)
    assert rows["count"] >= 1000, "small_scene holds 1 450 coloured rows"
    packed = ctx.download_result_packed().copy()
    for base in (-1, (1 << 32) - 100):
        with pytest.raises(capi.PcpError) as e:
            ctx.ortho_add(base)
        assert e.value.code == capi.PCP_ERR_RANGE
    assert ctx.ortho_stats()["adds"] == 0, "a refused add leaves the map as it was"
    added = ctx.ortho_add(0)
    # the restatement on the compacted rows, under their input indices
    n = len(s["x"])
    has = np.zeros(n, bool)
    has[rows["index"]] = True
    xyz = np.stack([s["x"], s["y"], s["z"]], axis=1)
    rgb = np.zeros((n, 3), np.uint8)
    rgb[rows["index"]] = rows["rgb"]
    label = np.zeros(n, np.uint8)
    label[rows["index"]] = rows["label"]
    assert xyz[rows["index"]].tobytes() == rows["xyz"].tobytes()
    want = ref.ortho(fr, xyz, rgb, label=label, has=has, fill_radius=3)
    assert added == want["contributors"] and want["occupied"] >= 500 and len(np.unique(want["label"])) >= 2
    # the adds change nothing else
    assert np.array_equal(ctx.download_result_packed(), packed)
    after = ctx.colour_compact(want_label=True)
    assert all(after[k].tobytes() == rows[k].tobytes() for k in ("index", "xyz", "rgb", "label"))
    # the accumulator survives a new upload, a colour reset and new frames
    ctx.upload_cloud(s["x"][:100], s["y"][:100], s["z"][:100])
    ctx.colour_reset()
    ctx.set_frames(s["poses"])
    assert ctx.ortho_finish(3) == (want["occupied"], want["filled"])
    _same(ctx.ortho_fetch(want_label=True), want, with_label=True)
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_add_packed(np.zeros(100, np.uint32))  # an add after a finish
    assert e.value.code == capi.PCP_ERR_STATE
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_finish(1025)
    assert e.value.code == capi.PCP_ERR_INVALID
    # the first add fixes whether labels are held
    ctx.ortho_begin(fr)
    ctx.ortho_add_packed(np.full(100, 0x01FFFFFF, np.uint32))
    ctx.ortho_finish(0)
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_fetch(want_label=True)
    assert e.value.code == capi.PCP_ERR_STATE
    # an empty map stays empty whatever the radius
    ctx.ortho_begin(ref.down_frame(0.05, d_min=50.0))
    assert ctx.ortho_add_packed(np.full(100, 0x01FFFFFF, np.uint32)) == 0
    assert ctx.ortho_finish(7) == (0, 0)
    got = ctx.ortho_fetch()
    assert (got["index"] == 0xFFFFFFFF).all() and (got["source"] == -1).all() and not got["status"].any() and not got["depth"].any()
    # the frame rules hold on the device path too, and a refused begin keeps the map that was live
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_begin(dict(fr, n=[0.0, 0.0, 1.0]))
    assert e.value.code == capi.PCP_ERR_INVALID
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_begin(dict(fr, width=16385))
    assert e.value.code == capi.PCP_ERR_RANGE and "fits at gsd" in str(e.value)
    assert ctx.ortho_stats()["pixels"] == fr["width"] * fr["height"]
    ctx.ortho_end()
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_stats()
    assert e.value.code == capi.PCP_ERR_STATE


def test_mask_edt_is_unchanged_by_a_fill(gpu_ctx_factory, small_scene):
    """the distance maps share k_md_columns / k_md_rows with the fill, which brings its own scratch"""
    from pointcloudprocessor_amd import capi

    s = small_scene
    b = _base(gpu_ctx_factory)
    ctx = gpu_ctx_factory()
    _views(ctx, capi, s)
    before = ctx.mask_edt(2)
    host = capi.mask_edt_host(s["masks"][2], 0)
    assert np.array_equal(before["d2"], host["d2"]) and np.array_equal(before["nearest"], host["nearest"])
    sc = b["scene"]
    ctx.upload_cloud(sc["xyz"][:, 0], sc["xyz"][:, 1], sc["xyz"][:, 2])
    fr = ref.down_frame(0.02)
    got, _, _, _ = _map(ctx, fr, sc["words"], 4)
    _same(got, _want(b, (0.02, 4), fr, 4))
    after = ctx.mask_edt(2)
    assert after["d2"].tobytes() == before["d2"].tobytes() and after["nearest"].tobytes() == before["nearest"].tobytes()
    _same(ctx.ortho_fetch(), _want(b, (0.02, 4), fr, 4))  # and the map is untouched by the distance maps
    ctx.ortho_end()
