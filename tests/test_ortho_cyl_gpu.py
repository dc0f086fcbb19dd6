"""The unrolled maps of cylindrical facets on the device ("Cylindrical facets") against the restatement in
_ortho_cyl_ref.py.  Every comparison is exact equality.

The base upload is one coaxial scene under the rotation of seed 5: a half cylinder (R 1, H 3, 20 000 points, 2 mm noise), a
closed ring inside it (R 0.4, H 2, 6 000 points), 300 exact copies of one point, two non-finite points, a point on the axis and
points on the octant boundaries and on both sides of the seam, seen from inside through frames of R = 1 whose raster is
shorter than the half cylinder and whose window ends 3 mm behind it.  The preconditions are asserted on the restatement's own
counts."""
import numpy as np
import pytest

import _ortho_cyl_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

SEED = 5
_BASE = {}


def _local_to_world(rot, local):
    return (np.asarray(local, np.float64) @ rot.T + ref.CENTRE).astype(np.float32)


def base_frame(gsd, rot, seam=0.3, height_m=2.6, d_min=-0.7, d_max=0.003, radius=1.0):
    """seen from inside: a = -z' (rows run down from h = +height_m / 2), theta from the seam direction towards a x e"""
    a = -rot[:, 2]
    e = np.cos(seam) * rot[:, 0] + np.sin(seam) * rot[:, 1]
    b = np.cross(a, e)  # side +1
    g = float(np.float32(gsd))
    c = ref.CENTRE + 0.5 * height_m * rot[:, 2]
    return ref.frame(c, a, e, b, radius, gsd, int(np.ceil(2 * np.pi * radius / g)), int(height_m / g), d_min, d_max, 1)


def base_scene():
    half = ref.cylinder_scene(20000, 1.0, 3.0, np.pi, 0.002, SEED)
    ring = ref.cylinder_scene(6000, 0.4, 2.0, 2 * np.pi, 0.002, SEED)  # (the same seed: the same rotation, so coaxial)
    rot = half["rot"]
    assert np.array_equal(rot, ring["rot"])
    copies = np.repeat(half["xyz"][123:124], 300, axis=0)
    odd = np.array([[np.nan, 0, 0], [1.0, np.inf, 2.0]], np.float32)
    on_axis = _local_to_world(rot, [[0.0, 0.0, 0.25]])
    # the octant boundaries of the frame's own angle (seam at 0.3 rad) and both sides of each, and both sides of the seam, on R = 1
    # and R = 0.4; after the rotation and the cast they lie within a few float roundings of the boundaries, on either side
    ang = []
    for k in range(8):
        for d in (-3e-7, -1e-7, 0.0, 1e-7, 3e-7):
            ang.append(0.3 - k * np.pi / 4 + d)  # (the frame's theta runs against the scene's)
    ang = np.array(ang)
    marks = np.concatenate([np.stack([r * np.cos(ang), r * np.sin(ang), np.full(len(ang), hh)], axis=1) for r, hh in ((1.0, 0.5), (0.4, -0.5))])
    xyz = np.concatenate([half["xyz"], ring["xyz"], copies, odd, on_axis, _local_to_world(rot, marks)]).astype(np.float32)
    rgb = ref.hash_colours(len(xyz))
    has = (np.arange(len(xyz)) % 11 != 3)
    return dict(xyz=xyz, rgb=rgb, has=has, words=ref.words_of(rgb, has), rot=rot, copy_row=123, n_half=20000, n_ring=6000)


def _base(make):
    """the base scene uploaded once on a context of its own; the restatements by (gsd, R) are computed once and shared"""
    if not _BASE:
        s = base_scene()
        for v in s.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        ctx = make()
        ctx.upload_cloud(np.ascontiguousarray(s["xyz"][:, 0]), np.ascontiguousarray(s["xyz"][:, 1]), np.ascontiguousarray(s["xyz"][:, 2]))
        _BASE.update(ctx=ctx, scene=s, want={})
    return _BASE


def _want(b, key, fr, radius):
    if key not in b["want"]:
        s = b["scene"]
        w = ref.ortho(fr, s["xyz"], s["rgb"], has=s["has"], fill_radius=radius)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        b["want"][key] = w
    return b["want"][key]


def _map(ctx, fr, words, radius, index_base=0):
    ctx.ortho_begin_cyl(fr)
    added = ctx.ortho_add_packed(words, index_base)
    occupied, filled = ctx.ortho_finish(radius)
    return ctx.ortho_fetch(), added, occupied, filled


def _same(got, want, with_label=False):
    bad = ref.same(got, want, with_label)
    assert bad is None, f"{bad} differs"


def _upload(ctx, xyz):
    ctx.upload_cloud(np.ascontiguousarray(xyz[:, 0]), np.ascontiguousarray(xyz[:, 1]), np.ascontiguousarray(xyz[:, 2]))


@pytest.mark.parametrize("gsd", [0.01, 0.05])
def test_device_equals_the_restatement(gpu_ctx_factory, gsd):
    from pointcloudprocessor_amd import capi

    b = _base(gpu_ctx_factory)
    ctx, s = b["ctx"], b["scene"]
    fr = base_frame(gsd, s["rot"])
    cut_raster, cut_window = ref.cuts(fr, s["xyz"])
    for radius in (0, 2, 4):
        want = _want(b, (gsd, radius), fr, radius)
        pp = want["per_pixel"]
        print(f"gsd {gsd} R {radius}: raster {fr['width']} x {fr['height']} contributors {want['contributors']} occupied {want['occupied']} "
              f"multi {(pp >= 2).sum()} max {pp.max()} ties {want['ties']} filled {want['filled']} cut by raster {cut_raster} by window {cut_window}")
        assert (pp >= 2).sum() >= 100 and pp.max() >= 200 and want["ties"] >= 1 and cut_raster >= 100 and cut_window >= 100
        assert radius == 0 or want["filled"] >= 100
        got, added, occupied, filled = _map(ctx, fr, s["words"], radius)
        _same(got, want)
        assert (added, occupied, filled) == (want["contributors"], want["occupied"], want["filled"])
        st = ctx.ortho_stats()
        assert st["pixels"] == fr["width"] * fr["height"] and st["adds"] == 1 and 0 < st["atomics"] <= added
        if radius == 0:  # the host twin gives the same bytes
            host = capi.ortho_cyl_host(fr, s["xyz"], s["rgb"], has=s["has"].astype(np.uint8))
            _same(host, want)
    # both depths win pixels: the ring (0.6 m nearer) and the half cylinder behind it
    direct = want["status"] == 1
    assert (want["depth"][direct] < -0.5).sum() >= 100 and (want["depth"][direct] > -0.1).sum() >= 100
    ctx.ortho_end()


def test_exact_octant_boundaries_and_the_seam(gpu_ctx_factory):
    """an axis-parallel frame, where s and t are exact: S = +-T, S = +-0, T = +-0 and one float on either side of each"""
    fr = ref.frame((0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, 0), 1.0, 0.01, 629, 200, -0.5, 0.5, -1)
    pts = []
    one = np.float32(1.0)
    up, down = np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))
    tiny = np.float32(1e-45)
    for sx in (1, -1):
        for sy in (1, -1):
            for u, v in ((one, one), (up, one), (down, one), (one, np.float32(0)), (np.float32(0), one), (one, tiny), (tiny, one),
                         (one, np.float32(0.41421357)), (one, np.float32(0.41421354)), (np.float32(0.41421357), one)):
                pts.append((sx * u, sy * v, 0.5))
    pts += [(1.0, -0.0, 0.25), (-1.0, -0.0, 0.25), (-0.0, 1.0, 0.25), (0.0, 0.0, 0.5), (-0.0, -0.0, 0.5)]
    xyz = np.array(pts, np.float32)
    rgb = ref.hash_colours(len(xyz))
    want = ref.ortho(fr, xyz, rgb, fill_radius=1)
    ok, pixel, _ = ref.project(fr, xyz)
    cols = pixel[ok] % fr["width"]
    assert want["contributors"] == int(ok.sum()) >= 30 and not ok[-2:].any(), "the two points on the axis do not contribute"
    assert cols.min() == 0 and cols.max() == 628 and len(np.unique(cols)) >= 12, "columns on both sides of the seam"
    ctx = gpu_ctx_factory()
    _upload(ctx, xyz)
    got, added, _, _ = _map(ctx, fr, ref.words_of(rgb), 1)
    _same(got, want)
    assert added == want["contributors"]
    ctx.ortho_end()
    ctx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_smallest_shapes_of_the_wavefront_merge(gpu_ctx_factory, n):
    b = _base(gpu_ctx_factory)
    rot = b["scene"]["rot"]
    fr = base_frame(0.05, rot, d_max=0.05)
    rng = np.random.default_rng(n)
    ctx = gpu_ctx_factory()
    for alternate in (False, True):
        # pixel centres (column 40 or 47, row 20) at radii of a few distinct depths, some of them repeated
        col = np.where(alternate & (np.arange(n) % 2 == 1), 47.5, 40.5)
        theta = col * fr["gsd"] / 1.0
        rad = 1.0 - 0.001 * rng.integers(0, 5, n)
        ang = 0.3 - theta  # (the frame's theta runs against the scene's)
        local = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(n, 1.3 - 20.5 * fr["gsd"])], axis=1)
        xyz = _local_to_world(rot, local)
        rgb = ref.hash_colours(n)
        want = ref.ortho(fr, xyz, rgb)
        assert want["contributors"] == n and want["occupied"] == (2 if alternate and n > 1 else 1)
        _upload(ctx, xyz)
        got, added, occupied, _ = _map(ctx, fr, ref.words_of(rgb), 0)
        _same(got, want)
        st = ctx.ortho_stats()
        assert (added, occupied) == (n, want["occupied"]) and want["occupied"] <= st["atomics"] <= n
    ctx.ortho_end()
    ctx.close()


def test_order_independence(gpu_ctx_factory):
    b = _base(gpu_ctx_factory)
    s = b["scene"]
    fr = base_frame(0.05, s["rot"])
    want = _want(b, (0.05, 2), fr, 2)
    n = len(s["xyz"])
    ctx = gpu_ctx_factory()
    perm = np.random.default_rng(21).permutation(n)
    xyz, rgb, words = s["xyz"][perm], s["rgb"][perm], s["words"][perm]
    _upload(ctx, xyz)
    got, _, _, _ = _map(ctx, fr, words, 2)
    _same(got, ref.ortho(fr, xyz, rgb, has=s["has"][perm], fill_radius=2))
    for k in ("depth", "status", "source"):  # what does not name a row is the unpermuted map's
        assert got[k].tobytes() == want[k].tobytes(), k
    half = n // 2
    parts = [(0, half), (half, n)]
    for order in (parts, parts[::-1]):
        ctx.ortho_begin_cyl(fr)
        added = 0
        for a, z in order:
            _upload(ctx, s["xyz"][a:z])
            added += ctx.ortho_add_packed(s["words"][a:z], index_base=a)
        assert ctx.ortho_finish(2) == (want["occupied"], want["filled"]) and added == want["contributors"]
        _same(ctx.ortho_fetch(), want)
        assert ctx.ortho_stats()["adds"] == 2
    import torch

    dev = torch.from_numpy(s["words"][half:n].view(np.int32).copy()).to("cuda:0")  # (the same 32 bits)
    torch.cuda.synchronize()
    ctx.ortho_begin_cyl(fr)
    _upload(ctx, s["xyz"][half:])
    ctx.ortho_add_packed(int(dev.data_ptr()), index_base=half)
    _upload(ctx, s["xyz"][:half])
    ctx.ortho_add_packed(s["words"][:half], index_base=0)
    ctx.ortho_finish(2)
    _same(ctx.ortho_fetch(), want)
    ctx.ortho_end()
    ctx.close()


def _views(ctx, capi, s):
    ctx.set_camera(cam_struct(capi, s["cam"]))
    e = np.zeros(0, np.float32)
    ctx.upload_cloud(e, e, e)
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
        ctx.upload_mask(f, s["masks"][f])


def _room_frame(gsd=0.05):
    """a cylinder of R = 5 about the vertical through the room's middle, seen from inside"""
    return ref.frame((0, 0, 4), (0, 0, -1), (1, 0, 0), (0, -1, 0), 5.0, gsd, int(np.ceil(2 * np.pi * 5.0 / gsd)), int(5.0 / gsd), -5.0, 5.0, 1)


def test_add_facet_the_state_rules_and_nothing_else_changes(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    import _ortho_ref as oref

    s = small_scene
    xyz = np.stack([s["x"], s["y"], s["z"]], axis=1).astype(np.float32)
    prm = dict(link_radius=0.5, angle_deg=10.0, plane_tol=0.01, max_curvature=0.01, min_points=50)

    def coloured():
        ctx = gpu_ctx_factory()
        _views(ctx, capi, s)
        ctx.set_label_fusion(True)
        ctx.upload_cloud(s["x"], s["y"], s["z"])
        ctx.colorize(download=False)
        return ctx

    ctx = coloured()
    packed = ctx.download_result_packed().copy()
    labels = ctx.colour_labels()
    ctx.crack_fuse_begin()
    for f in range(3):
        ctx.crack_fuse_add(f)
    cracks = ctx.crack_components(1, 0.05)
    ctx.estimate_normals(0.5)
    normals = ctx.normals_fetch()
    fac = ctx.facets(**prm)
    has = (packed >> 24).astype(np.uint8)
    rgb = np.stack([packed & 0xFF, (packed >> 8) & 0xFF, (packed >> 16) & 0xFF], axis=1).astype(np.uint8)
    per = np.array([int(((fac["label"] == fid) & (has > 0)).sum()) for fid in fac["ids"]])
    fid = int(fac["ids"][np.argmax(per)])
    member = fac["label"] == fid
    assert per.max() >= 100 and ((has > 0) & ~member).sum() >= 100, "the filter has rows to keep and rows to leave out"
    cyl, plane = _room_frame(), oref.down_frame(0.05)
    # ortho_add_facet and ortho_add under a cylinder's frame against the host twin
    for radius in (0, 3):
        want = capi.ortho_cyl_host(cyl, xyz, rgb, label=labels["label"], has=(has > 0) & member, fill_radius=radius)
        ctx.ortho_begin_cyl(cyl)
        added = ctx.ortho_add_facet(fid)
        occupied, filled = ctx.ortho_finish(radius)
        got = ctx.ortho_fetch(want_label=True)
        assert (added, occupied, filled) == (want["contributors"], want["occupied"], want["filled"]) and occupied >= 50
        _same(got, want, with_label=True)
    whole_want = capi.ortho_cyl_host(cyl, xyz, rgb, label=labels["label"], has=has, fill_radius=0)
    ctx.ortho_begin_cyl(cyl)
    whole_added = ctx.ortho_add(0)
    assert whole_added == whole_want["contributors"] > added
    ctx.ortho_finish(0)
    whole = ctx.ortho_fetch(want_label=True)
    _same(whole, whole_want, with_label=True)
    # the state: an add after the finish; the orthophoto refused by name; a refused begin of either kind leaves the live map
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_add(0)
    assert e.value.code == capi.PCP_ERR_STATE and "finished" in str(e.value)
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_texture(2)
    assert e.value.code == capi.PCP_ERR_STATE and "orthophotos of unrolled maps are not built" in str(e.value)
    for begin, bad, code in ((ctx.ortho_begin_cyl, dict(cyl, side=0), capi.PCP_ERR_INVALID),
                             (ctx.ortho_begin_cyl, dict(cyl, width=cyl["width"] + 2), capi.PCP_ERR_INVALID),
                             (ctx.ortho_begin_cyl, dict(cyl, radius=900.0, width=16385), capi.PCP_ERR_RANGE),
                             (ctx.ortho_begin, dict(plane, gsd=2.0), capi.PCP_ERR_INVALID)):
        with pytest.raises(capi.PcpError) as e:
            begin(bad)
        assert e.value.code == code
        again = ctx.ortho_fetch(want_label=True)
        assert again["index"].shape == (cyl["height"], cyl["width"])
        _same(again, whole_want, with_label=True)
    # planar after cylindrical equals a fresh context's, and cylindrical after planar again the first
    flat_want = capi.ortho_host(plane, xyz, rgb, label=labels["label"], has=has, fill_radius=2)
    ctx.ortho_begin(plane)
    assert ctx.ortho_add(0) == flat_want["contributors"]
    ctx.ortho_finish(2)
    flat = ctx.ortho_fetch(want_label=True)
    fresh = coloured()
    fresh.ortho_begin(plane)
    fresh.ortho_add(0)
    fresh.ortho_finish(2)
    again = fresh.ortho_fetch(want_label=True)
    fresh.ortho_end()
    fresh.close()
    for k in ("index", "depth", "rgb", "label", "status", "source"):
        assert flat[k].tobytes() == again[k].tobytes() == flat_want[k].tobytes(), k
    ctx.ortho_begin_cyl(cyl)
    ctx.ortho_add(0)
    ctx.ortho_finish(0)
    _same(ctx.ortho_fetch(want_label=True), whole_want, with_label=True)
    ctx.ortho_end()
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_stats()
    assert e.value.code == capi.PCP_ERR_STATE
    # nothing else changed
    assert np.array_equal(ctx.download_result_packed(), packed)
    after = ctx.colour_labels()
    assert all(after[k].tobytes() == labels[k].tobytes() for k in labels)
    cr = ctx.crack_components(1, 0.05)
    assert all(np.asarray(cr[k]).tobytes() == np.asarray(cracks[k]).tobytes() for k in cracks)
    assert np.array_equal(ctx.facets_fetch()["ids"], fac["ids"])
    now = ctx.normals_fetch()
    assert all(np.asarray(now[k]).tobytes() == np.asarray(normals[k]).tobytes() for k in normals)
    ctx.crack_fuse_end()
    ctx.close()
