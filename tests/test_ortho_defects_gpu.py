"""The surface defects on ortho maps on the device ("Surface defects on ortho maps") against the restatement in
_ortho_defects_ref.py, bit for bit: the three layers, the eight counts, the table.

A map with a wanted depth field comes from one point per pixel under the frame o = 0, u = +x, v = +y, n = +z at a gsd of
2^-7 m: the point ((c + 1/2) gsd, (r + 1/2) gsd, d) lands on pixel (r, c) with depth d exactly.  Pixels of status 0 and NaN
depths get no point (a NaN cannot enter a map: OM2 refuses the point; the CPU suite covers SD2's NaN), and where the raster
wants filled pixels the map is finished with a fill radius of 1, so pixels next to a measured one are filled and the inside
of the carved blocks stays empty.  The restatement always runs on the layers the finished map gives back."""
import numpy as np
import pytest

import _ortho_cyl_ref as cref
import _ortho_defects_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

GSD = 2.0 ** -7
CASES = ref.cases()
_CTX = {}


def _ctx(make):
    if "ctx" not in _CTX:
        _CTX["ctx"] = make()
    return _CTX["ctx"]


def _frame(h, w):
    return dict(o=(0.0, 0.0, 0.0), u=(1.0, 0.0, 0.0), v=(0.0, 1.0, 0.0), n=(0.0, 0.0, 1.0), gsd=GSD, width=w, height=h, d_min=-1000.0,
                d_max=1000.0)


def _points(depth, status):
    rr, cc = np.nonzero((status == 1) & np.isfinite(depth))
    return np.stack([(cc + 0.5) * GSD, (rr + 0.5) * GSD, depth[rr, cc]], axis=1).astype(np.float32)


def _upload(ctx, xyz):
    ctx.upload_cloud(np.ascontiguousarray(xyz[:, 0]), np.ascontiguousarray(xyz[:, 1]), np.ascontiguousarray(xyz[:, 2]))


def _map(ctx, depth, status, fill=0):
    """the finished planar map of a raster: its fetched layers"""
    xyz = _points(depth, status)
    _upload(ctx, xyz)
    h, w = depth.shape
    ctx.ortho_begin(_frame(h, w))
    assert ctx.ortho_add_packed(np.full(len(xyz), 0x01808080, np.uint32)) == len(xyz)
    ctx.ortho_finish(fill)
    return ctx.ortho_fetch()


def _device(ctx, **kw):
    out = ctx.ortho_defects(**kw)
    got = ctx.ortho_defects_fetch()
    got["rows"] = ctx.ortho_defects_table()
    got["out"] = np.array([out[k] for k in ref.OUT], np.int64)
    return got


def _carve(spec, depth, status):
    """random rasters: blocks of empty pixels that a fill of radius 1 cannot close, and every status-2 pixel left to the fill"""
    if spec[0] != "random":
        return depth, status, int((status == 2).any())
    status = status.copy()
    h, w = status.shape
    if h >= 20 and w >= 20:
        status[h // 3:h // 3 + 6, w // 4:w // 4 + 7] = 0
        status[0:4, w - 5:w] = 0
    return depth, status, 1


@pytest.mark.parametrize("name,spec,kw", CASES, ids=[c[0] for c in CASES])
def test_device_equals_the_restatement(gpu_ctx_factory, name, spec, kw):
    ctx = _ctx(gpu_ctx_factory)
    depth, status, fill = _carve(spec, *ref.raster(spec))
    m = _map(ctx, depth, status, fill)
    if fill == 0:  # the map is the raster
        assert np.array_equal(m["status"], status) and np.array_equal(m["depth"], depth)
    elif spec[0] != "random":  # ... but for the hole's rim, which the fill closes
        assert (m["status"][status == 1] == 1).all() and (m["status"] == 0).sum() == 2 and (m["status"] == 2).sum() == 11
    want = ref.defects(m["depth"], m["status"], **kw)
    print(name, dict(zip(ref.OUT, want["out"])), "status", np.bincount(m["status"].ravel(), minlength=3))
    if spec[:3] == ("random", 202, 242):  # the preconditions of the large raster, on the map's own layers
        assert all((m["status"] == k).sum() >= 30 for k in (0, 1, 2)) and want["out"][5] >= 1
        assert want["out"][0] >= 50 and want["out"][1] >= 50 and want["out"][2] >= 300 and want["out"][3] >= 300
    got = _device(ctx, **kw)
    assert ref.same(got, want) is None, ref.same(got, want)
    again = ctx.ortho_fetch()
    for k in m:
        assert np.array_equal(m[k], again[k], equal_nan=m[k].dtype.kind == "f"), k  # SD8: the map is never modified


def test_paging_of_the_table(gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    depth, status = ref.raster(("random", 60, 70))
    m = _map(ctx, depth, status, 0)
    want = ref.defects(m["depth"], m["status"])
    ctx.ortho_defects()
    n = len(want["rows"])
    assert n > 5
    assert np.array_equal(ctx.ortho_defects_table(2, 3), want["rows"][2:5])
    assert np.array_equal(ctx.ortho_defects_table(n - 1, 10), want["rows"][n - 1:])
    assert ctx.ortho_defects_table(n, 10).shape == (0, 16) and ctx.ortho_defects_table(0, 0).shape == (0, 16)


def test_state_rules(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi

    ctx = gpu_ctx_factory()
    fresh = (ctx.ortho_defects, ctx.ortho_defects_fetch, ctx.ortho_defects_table)
    for call in fresh:  # no map at all
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_STATE
    with pytest.raises(capi.PcpError) as e:  # the parameters are checked before the state
        ctx.ortho_defects(threshold=2.0)
    assert e.value.code == capi.PCP_ERR_INVALID and "threshold" in str(e.value)
    depth, status = ref.edge_and_hole()
    xyz = _points(depth, status)
    _upload(ctx, xyz)
    ctx.ortho_begin(_frame(*depth.shape))
    ctx.ortho_add_packed(np.full(len(xyz), 0x01808080, np.uint32))
    with pytest.raises(capi.PcpError) as e:  # not finished
        ctx.ortho_defects()
    assert e.value.code == capi.PCP_ERR_STATE and "pcp_ortho_finish" in str(e.value)
    ctx.ortho_finish(0)
    with pytest.raises(capi.PcpError) as e:  # finished, no results yet
        ctx.ortho_defects_fetch()
    assert e.value.code == capi.PCP_ERR_STATE
    m = ctx.ortho_fetch()
    first = _device(ctx)
    assert ref.same(first, ref.defects(m["depth"], m["status"])) is None and first["out"][0] == 2
    # results replaced by a second call
    second = _device(ctx, classes=2, window=3, min_support=2)
    assert ref.same(second, ref.defects(m["depth"], m["status"], classes=2, window=3, min_support=2)) is None
    assert ref.same(second, first) is not None
    # a refused call leaves the earlier results
    for kw in (dict(window=-1), dict(classes=0), dict(window=0, refine=True), dict(min_pixels=0), dict(window=2, min_support=0)):
        with pytest.raises(capi.PcpError) as e:
            ctx.ortho_defects(**kw)
        assert e.value.code == capi.PCP_ERR_INVALID
    kept = ctx.ortho_defects_fetch()
    assert all(np.array_equal(kept[k], second[k]) for k in kept) and np.array_equal(ctx.ortho_defects_table(), second["rows"])
    # results dropped by _finish (also one that changes nothing), by either begin and by _end
    ctx.ortho_finish(0)
    for call in (ctx.ortho_defects_fetch, ctx.ortho_defects_table):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_STATE
    assert ctx.ortho_defects()["kept"] == 2
    ctx.ortho_begin(_frame(*depth.shape))
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_defects_fetch()
    assert e.value.code == capi.PCP_ERR_STATE
    ctx.ortho_add_packed(np.full(len(xyz), 0x01808080, np.uint32))
    ctx.ortho_finish(0)
    assert ctx.ortho_defects()["kept"] == 2
    ctx.ortho_end()
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_defects_table()
    assert e.value.code == capi.PCP_ERR_STATE
    L = capi.load()
    assert L.pcp_ortho_defects(None, None, None) == capi.PCP_ERR_INVALID and L.pcp_ortho_defects(ctx.h, None, None) == capi.PCP_ERR_INVALID


def test_a_map_without_surface_pixels(gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    _upload(ctx, np.array([[5.0, 5.0, 0.0]], np.float32))  # outside the raster
    ctx.ortho_begin(_frame(9, 17))
    assert ctx.ortho_add_packed(np.full(1, 0x01808080, np.uint32)) == 0
    ctx.ortho_finish(2)
    m = ctx.ortho_fetch()
    for kw in (dict(), dict(window=3, refine=True)):
        got = _device(ctx, **kw)
        assert ref.same(got, ref.defects(m["depth"], m["status"], **kw)) is None
        assert not got["out"].any() and got["rows"].shape == (0, 16) and not got["cls"].any() and not got["region"].any()


def test_mask_distance_maps_are_untouched(gpu_ctx_factory, small_scene):
    """the stage shares no scratch with the mask distance maps: pcp_mask_edt bit for bit before and after"""
    from pointcloudprocessor_amd import capi

    ctx = gpu_ctx_factory()
    ctx.set_camera(cam_struct(capi, small_scene["cam"]), capi.default_cull_params())
    depth, status = ref.raster(("random", 60, 70))
    xyz = _points(depth, status)
    _upload(ctx, xyz)
    ctx.set_frames(small_scene["poses"])
    ctx.upload_mask(0, small_scene["masks"][0])
    before = ctx.mask_edt(0)
    ctx.ortho_begin(_frame(*depth.shape))
    ctx.ortho_add_packed(np.full(len(xyz), 0x01808080, np.uint32))
    ctx.ortho_finish(1)
    m = ctx.ortho_fetch()
    got = _device(ctx, window=7, refine=True, min_support=3)
    assert ref.same(got, ref.defects(m["depth"], m["status"], window=7, refine=True, min_support=3)) is None
    after, again = ctx.mask_edt(0), ctx.ortho_fetch()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert all(np.array_equal(m[k], again[k], equal_nan=m[k].dtype.kind == "f") for k in m)


@pytest.mark.parametrize("side", [1, -1])
def test_a_dent_on_a_cylinder_reads_as_a_hollow_from_either_side(gpu_ctx_factory, side):
    """CY2: depth = side (rho - R).  A dent is material missing as the viewer sees it: rho grows for the viewer inside (side +1),
    shrinks for the viewer outside (side -1); either way the depth is positive and the class 1.  A boss is the opposite."""
    ctx = _ctx(gpu_ctx_factory)
    R, g, h, w = 1.0, 0.01, 40, 60
    a, e = np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0])
    b = side * np.cross(a, e)
    fr = cref.frame((0.0, 0.0, 1.0), a, e, b, R, g, w, h, -0.5, 0.5, side)
    rr, cc = np.mgrid[0:h, 0:w]
    depth = np.zeros((h, w))
    depth[10:16, 8:20] = 0.008   # the dent
    depth[25:30, 35:50] = -0.006  # the boss
    theta, hh, rho = (cc + 0.5) * g / R, (rr + 0.5) * g, R + side * depth
    xyz = (np.array([0.0, 0.0, 1.0]) + (rho * np.cos(theta))[..., None] * e + (rho * np.sin(theta))[..., None] * b + hh[..., None] * a)
    xyz = xyz.reshape(-1, 3).astype(np.float32)
    _upload(ctx, xyz)
    ctx.ortho_begin_cyl(fr)
    assert ctx.ortho_add_packed(np.full(len(xyz), 0x01808080, np.uint32)) == len(xyz)
    ctx.ortho_finish(0)
    m = ctx.ortho_fetch()
    assert (m["status"] == 1).all()
    got = _device(ctx, threshold=0.003)
    assert ref.same(got, ref.defects(m["depth"], m["status"], threshold=0.003)) is None
    assert got["out"][0] == 2 and list(got["rows"][:, ref.R_CLASS]) == [1, 2]
    dent, boss = got["rows"]
    assert dent[ref.R_PIXELS] == 6 * 12 and (dent[ref.R_COL_MIN], dent[ref.R_COL_MAX], dent[ref.R_ROW_MIN], dent[ref.R_ROW_MAX]) == (8, 19, 10, 15)
    assert boss[ref.R_PIXELS] == 5 * 15 and abs(dent[ref.R_MAX] / ref.Q - 0.008) < 1e-5 and abs(boss[ref.R_MAX] / ref.Q - 0.006) < 1e-5


@pytest.mark.parametrize("gsd", [0.004, 0.002])
def test_cap_scene_meets_its_analytic_values(gpu_ctx_factory, gsd):
    """the CPU suite's cap scene through the device's map and the device's stage: the same bounds"""
    ctx = _ctx(gpu_ctx_factory)
    xyz = ref.cap_scene(gsd)
    _upload(ctx, xyz)
    ctx.ortho_begin(ref.cap_frame(gsd))
    ctx.ortho_add_packed(np.full(len(xyz), 0x01808080, np.uint32))
    occupied, filled = ctx.ortho_finish(0)
    m = ctx.ortho_fetch()
    assert occupied == m["depth"].size and filled == 0
    got = _device(ctx, threshold=ref.CAP_T)
    assert ref.same(got, ref.defects(m["depth"], m["status"], threshold=ref.CAP_T)) is None
    band, volume_bound, depth_bound = ref.cap_bounds(gsd)
    measures = ref.cap_measures(got["rows"], gsd)
    assert [k for k, _, _, _ in measures] == [1, 2]
    for k, area, volume, depth in measures:
        print(f"gsd {gsd} class {k}: area off by {(area - ref.CAP_AREA) / band:+.3f} of the band, volume by "
              f"{(volume - ref.CAP_VOLUME) / ref.CAP_VOLUME:+.4f} (bound {volume_bound}), greatest depth by {depth - ref.CAP_H:+.2e} m (bound {depth_bound:.2e})")
        assert abs(area - ref.CAP_AREA) <= band
        assert abs(volume - ref.CAP_VOLUME) <= volume_bound * ref.CAP_VOLUME
        assert abs(depth - ref.CAP_H) <= depth_bound
    if gsd == 0.004:  # SD4 on the same map
        deep = {}
        for refine in (False, True):
            got = _device(ctx, threshold=ref.CAP_T, window=40, refine=refine)
            assert ref.same(got, ref.defects(m["depth"], m["status"], threshold=ref.CAP_T, window=40, refine=refine)) is None
            deep[refine] = {int(r[ref.R_CLASS]): r[ref.R_MAX] / ref.Q for r in got["rows"]}
        print("greatest depth, W = 40:", deep)
        for k in (1, 2):
            assert abs(deep[True][k] - ref.CAP_H) < abs(deep[False][k] - ref.CAP_H)
