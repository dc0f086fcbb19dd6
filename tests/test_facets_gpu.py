"""The planar facets on the device ("Planar facets") against the restatement in _facets_ref.py, which is fed the
normals and curvatures pcp_normals_fetch returns: labels, counts, ids, the ten integers and the boxes by exact equality.

The base scene is synth.make_cloud(60000) -- a room of 12 x 10 x 4 m with six spheres and four pillars, 1 mm of noise along the
normal -- after estimate_normals(0.3); parameters link 0.25, angle 10, tol 0.01, curvature 0.01, min_points 150.  What the scene
must give is asserted as a condition: the six largest facets are the room's faces."""
import numpy as np
import pytest

import _facets_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

BASE = dict(link_radius=0.25, angle_deg=10.0, plane_tol=0.01, max_curvature=0.01, min_points=150)
_SCENES = {}


def _scene(make, n, normal_radius=0.3):
    """make_cloud(n) uploaded on a context of its own with its normals estimated, once; restatements by parameters are shared"""
    if n not in _SCENES:
        from pointcloudprocessor_amd import synth

        x, y, z, _ = synth.make_cloud(n)
        xyz = np.stack([x, y, z], axis=1).astype(np.float32)
        ctx = make()
        ctx.upload_cloud(x, y, z)
        ctx.estimate_normals(normal_radius)
        nf = ctx.normals_fetch()
        for a in (xyz, nf["normal"], nf["curvature"]):
            a.setflags(write=False)
        _SCENES[n] = dict(ctx=ctx, xyz=xyz, normal=nf["normal"], curv=nf["curvature"], want={})
    return _SCENES[n]


def _want(s, **prm):
    key = tuple(sorted(prm.items()))
    if key not in s["want"]:
        w = ref.facets(s["xyz"], s["normal"], s["curv"], **prm)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        s["want"][key] = w
    return s["want"][key]


def _same(got, want):
    for k in ("facet_points", "components", "facets"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got["label"], want["label"])
    assert np.array_equal(got["ids"], want["ids"])
    assert np.array_equal(got["rows"], want["rows"])
    assert got["box"].tobytes() == want["box"].tobytes()


@pytest.mark.parametrize("n,link", [(60000, 0.25), (60000, 0.1), (60001, 0.25)])
def test_device_equals_the_restatement(gpu_ctx_factory, n, link):
    s = _scene(gpu_ctx_factory, n)
    prm = dict(BASE, link_radius=link)
    want = _want(s, **prm)
    print(f"n {n} link {link}: facet points {want['facet_points']} components {want['components']} facets {want['facets']} "
          f"largest {want['rows'][:, 0].max() if want['facets'] else 0}")
    assert want["facet_points"] > n // 2 and want["components"] > want["facets"] >= 1
    got = s["ctx"].facets(**prm)
    _same(got, want)
    # the fetch in windows
    part = s["ctx"].facets_fetch(1, 2)
    assert np.array_equal(part["ids"], want["ids"][1:3]) and np.array_equal(part["rows"], want["rows"][1:3])
    assert len(s["ctx"].facets_fetch(want["facets"], 5)["ids"]) == 0


def test_the_six_largest_facets_are_the_faces_of_the_room(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi

    s = _scene(gpu_ctx_factory, 60000)
    got = s["ctx"].facets(**BASE)
    planes = np.array([capi.facet_plane_host(s["xyz"][fid], row) for fid, row in zip(got["ids"], got["rows"])])
    order = np.argsort(-got["rows"][:, 0])
    for r in order:
        print(f"facet {got['ids'][r]}: {got['rows'][r, 0]} points rms {planes[r, 6]:.6f} normal {planes[r, 3:6]}")
    axes = set()
    for r in order[:6]:
        assert got["rows"][r, 0] > 3000
        assert 0.0005 <= planes[r, 6] <= 0.002  # 1 mm of noise along the normal; the quantum adds under 0.1 mm
        a = int(np.argmax(np.abs(planes[r, 3:6])))
        assert planes[r, 3 + a] >= np.cos(np.deg2rad(1.0))
        # which face: the axis and the side of the room the centroid lies on
        axes.add((a, bool(planes[r, a] > (2.0 if a == 2 else 0.0))))
    assert len(axes) == 6, axes
    # the sphere pieces: walked round by the local rule, flagged by the global one
    big = got["rows"][:, 0] > 150
    assert (planes[big, 6] > 0.1).sum() >= 1


def _run(make, xyz, normal_radius, **prm):
    ctx = make()
    ctx.upload_cloud(np.ascontiguousarray(xyz[:, 0]), np.ascontiguousarray(xyz[:, 1]), np.ascontiguousarray(xyz[:, 2]))
    ctx.estimate_normals(normal_radius)
    nf = ctx.normals_fetch()
    got = ctx.facets(**prm)
    want = ref.facets(xyz, nf["normal"], nf["curvature"], **prm)
    _same(got, want)
    return ctx, got


def test_edge_case_clouds(gpu_ctx_factory):
    from pointcloudprocessor_amd import synth

    prm = dict(link_radius=0.05, angle_deg=10.0, plane_tol=0.01, max_curvature=0.02, min_points=10)
    # every point the same: one cell, no plane to estimate, so no facet point
    dup = np.tile(np.array([[1.25, -2.5, 0.75]], np.float32), (5000, 1))
    ctx, got = _run(gpu_ctx_factory, dup, 0.05, **prm)
    assert got["facets"] == 0 and (got["label"] == -1).all()
    ctx.close()
    # 1 500 points of a 4 mm patch: one cell, every pair a candidate, one facet
    rng = np.random.default_rng(11)
    patch = np.concatenate([rng.random((1500, 2)) * 0.004, rng.normal(0.0, 2e-5, (1500, 1))], axis=1).astype(np.float32) + np.float32(3.0)
    ctx, got = _run(gpu_ctx_factory, patch, 0.05, **prm)
    assert got["facets"] == 1 and got["rows"][0, 0] == 1500 and (got["label"] == 0).all()
    ctx.close()
    # 300 exact copies and two non-finite points
    x, y, z, _ = synth.make_cloud(20000)
    xyz = np.stack([x, y, z], axis=1).astype(np.float32)
    xyz = np.concatenate([xyz, xyz[rng.integers(0, len(xyz), 300)]])
    xyz[17] = [np.nan, 0.0, 1.0]
    xyz[4711] = [1.0, np.inf, 1.0]
    wide = dict(link_radius=0.5, angle_deg=10.0, plane_tol=0.01, max_curvature=0.01, min_points=50)
    ctx, got = _run(gpu_ctx_factory, xyz, 0.5, **wide)
    assert got["facets"] >= 6 and got["label"][17] == -1 and got["label"][4711] == -1
    # no facet point at all: a curvature bound of zero on noisy data
    none = ctx.facets(**dict(wide, max_curvature=0.0))
    assert none["facet_points"] == 0 and none["facets"] == 0 and len(none["ids"]) == 0 and (none["label"] == -1).all()
    ctx.close()


def test_many_small_sheets_in_one_wavefront(gpu_ctx_factory):
    """200 sheets of 0.1 x 0.1 m half a metre apart, 70 points each and every tenth one 60: a wavefront of the cell order holds
    several rows, a few hold one; with min_points 64 the sheets of 60 are no facets"""
    rng = np.random.default_rng(12)
    parts = []
    for k in range(200):
        m = 60 if k % 10 == 9 else 70
        p = np.concatenate([rng.random((m, 2)) * 0.1, rng.normal(0.0, 1e-4, (m, 1))], axis=1)
        parts.append(p + np.array([0.5 * (k % 20), 0.5 * (k // 20), 0.0]))
    xyz = np.concatenate(parts).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    ctx, got = _run(gpu_ctx_factory, xyz, 0.05, link_radius=0.05, angle_deg=10.0, plane_tol=0.01, max_curvature=0.02, min_points=64)
    print("components", got["components"], "facets", got["facets"], "sizes", np.unique(got["rows"][:, 0], return_counts=True))
    assert got["components"] >= 200 and 150 <= got["facets"] <= 180
    assert (got["rows"][:, 0] >= 64).all() and (got["label"] == -1).sum() >= 20 * 60
    ctx.close()


def test_the_partition_is_the_same_under_a_permuted_upload(gpu_ctx_factory):
    s = _scene(gpu_ctx_factory, 60000)
    old = s["ctx"].facets(**BASE)
    n = len(s["xyz"])
    perm = np.random.default_rng(13).permutation(n)  # new row k = old row perm[k]
    xyz = s["xyz"][perm]
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(np.ascontiguousarray(xyz[:, 0]), np.ascontiguousarray(xyz[:, 1]), np.ascontiguousarray(xyz[:, 2]))
    ctx.estimate_normals(0.3)
    got = ctx.facets(**BASE)
    # (the normals are functions of the neighbour SETS, so they are the same bits under the permutation)
    assert ctx.normals_fetch()["curvature"].tobytes() == s["curv"][perm].tobytes()
    lab = old["label"][perm]
    inside = lab >= 0
    lowest = np.full(n, n, np.int64)
    np.minimum.at(lowest, lab[inside], np.flatnonzero(inside))
    want = np.full(n, -1, np.int64)
    want[inside] = lowest[lab[inside]]
    assert np.array_equal(got["label"], want)
    assert (got["facet_points"], got["components"], got["facets"]) == (old["facet_points"], old["components"], old["facets"])
    assert np.array_equal(np.sort(got["rows"][:, 0]), np.sort(old["rows"][:, 0]))
    ctx.close()


def test_state_rules(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi, synth

    x, y, z, _ = synth.make_cloud(5000)
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(x, y, z)
    prm = dict(link_radius=0.5, angle_deg=10.0, plane_tol=0.01, max_curvature=0.02, min_points=20)
    with pytest.raises(capi.PcpError) as e:
        ctx.facets(**prm)
    assert e.value.code == capi.PCP_ERR_STATE and "pcp_estimate_normals" in str(e.value)
    with pytest.raises(capi.PcpError) as e:
        ctx.facets_fetch()
    assert e.value.code == capi.PCP_ERR_STATE
    ctx.estimate_normals(0.5)
    with pytest.raises(capi.PcpError) as e:
        ctx.facets(**dict(prm, angle_deg=50.0))
    assert e.value.code == capi.PCP_ERR_INVALID and "angle_deg" in str(e.value)
    got = ctx.facets(**prm)
    assert got["facets"] >= 1 and len(ctx.facets_fetch()["ids"]) == got["facets"]
    with pytest.raises(capi.PcpError) as e:
        ctx.facets_fetch(-1, 1)
    assert e.value.code == capi.PCP_ERR_INVALID
    # a new estimate drops the table, and so does a new upload
    ctx.estimate_normals(0.4)
    with pytest.raises(capi.PcpError) as e:
        ctx.facets_fetch()
    assert e.value.code == capi.PCP_ERR_STATE
    ctx.facets(**prm)
    ctx.upload_cloud(x[:100], y[:100], z[:100])
    for call in (ctx.facets_fetch, lambda: ctx.facets(**prm)):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_STATE
    # an empty cloud: a table of no rows
    e0 = np.zeros(0, np.float32)
    ctx.upload_cloud(e0, e0, e0)
    ctx.estimate_normals(0.5)
    got = ctx.facets(**prm)
    assert got["facets"] == 0 and len(got["label"]) == 0 and len(ctx.facets_fetch()["ids"]) == 0
    ctx.close()


def _views(ctx, capi, s):
    ctx.set_camera(cam_struct(capi, s["cam"]))
    e = np.zeros(0, np.float32)
    ctx.upload_cloud(e, e, e)
    ctx.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        ctx.upload_image(f, im)
        ctx.upload_mask(f, s["masks"][f])


def test_ortho_add_facet_and_nothing_else_changes(gpu_ctx_factory, small_scene):
    from pointcloudprocessor_amd import capi

    s = small_scene
    xyz = np.stack([s["x"], s["y"], s["z"]], axis=1).astype(np.float32)
    n = len(xyz)
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
    visible = ctx.frame_visible(2)
    ctx.crack_fuse_begin()
    for f in range(3):
        ctx.crack_fuse_add(f)
    cracks = ctx.crack_components(1, 0.05)
    # no facets yet
    fr_any = capi.ortho_fit_frame_host(xyz, 0.05)
    ctx.ortho_begin(fr_any)
    with pytest.raises(capi.PcpError) as e:
        ctx.ortho_add_facet(0)
    assert e.value.code == capi.PCP_ERR_STATE and "pcp_facets" in str(e.value)
    ctx.estimate_normals(0.5)
    fac = ctx.facets(**prm)
    for bad in (-1, n):
        with pytest.raises(capi.PcpError) as e:
            ctx.ortho_add_facet(bad)
        assert e.value.code == capi.PCP_ERR_RANGE
    assert ctx.ortho_stats()["adds"] == 0
    ctx.ortho_end()
    has = (packed >> 24).astype(np.uint8)
    rgb = np.stack([packed & 0xFF, (packed >> 8) & 0xFF, (packed >> 16) & 0xFF], axis=1).astype(np.uint8)
    # the facet with the most coloured rows
    per = np.array([int(((fac["label"] == fid) & (has > 0)).sum()) for fid in fac["ids"]])
    fid = int(fac["ids"][np.argmax(per)])
    member = fac["label"] == fid
    print("facet", fid, "points", int(member.sum()), "coloured", int(per.max()), "of", int((has > 0).sum()))
    assert per.max() >= 100 and ((has > 0) & ~member).sum() >= 100, "the filter has rows to keep and rows to leave out"
    fr = capi.ortho_fit_frame_host(xyz, 0.05, has=member.astype(np.uint8))
    for radius in (0, 3):
        want = capi.ortho_host(fr, xyz, rgb, label=labels["label"], has=(has > 0) & member, fill_radius=radius)
        ctx.ortho_begin(fr)
        added = ctx.ortho_add_facet(fid)
        occupied, filled = ctx.ortho_finish(radius)
        got = ctx.ortho_fetch(want_label=True)
        ctx.ortho_end()
        assert (added, occupied, filled) == (want["contributors"], want["occupied"], want["filled"]) and occupied >= 50
        for k in ("index", "depth", "rgb", "label", "status", "source"):
            assert got[k].tobytes() == want[k].tobytes(), k
        if radius:
            assert filled > 0
    # the whole map through that frame holds more: rows of other facets fall into its window
    whole_want = capi.ortho_host(fr, xyz, rgb, label=labels["label"], has=has, fill_radius=0)
    ctx.ortho_begin(fr)
    whole_added = ctx.ortho_add(0)
    ctx.ortho_finish(0)
    whole = ctx.ortho_fetch(want_label=True)
    ctx.ortho_end()
    assert whole_added == whole_want["contributors"] and whole_added > added
    fresh = coloured()
    fresh.ortho_begin(fr)
    assert fresh.ortho_add(0) == whole_added
    fresh.ortho_finish(0)
    again = fresh.ortho_fetch(want_label=True)
    fresh.ortho_end()
    for k in ("index", "depth", "rgb", "label", "status", "source"):
        assert whole[k].tobytes() == again[k].tobytes() == whole_want[k].tobytes(), k
    # nothing else changed
    assert np.array_equal(ctx.download_result_packed(), packed)
    after = ctx.colour_labels()
    assert all(after[k].tobytes() == labels[k].tobytes() for k in labels)
    vis = ctx.frame_visible(2)
    assert all(np.asarray(vis[k]).tobytes() == np.asarray(visible[k]).tobytes() for k in visible)
    cr = ctx.crack_components(1, 0.05)
    assert all(np.asarray(cr[k]).tobytes() == np.asarray(cracks[k]).tobytes() for k in cracks)
    assert np.array_equal(ctx.facets_fetch()["ids"], fac["ids"]), "the crack stage rebuilt the grid; the facets' table stays"
    ctx.crack_fuse_end()
    ctx.close()
    fresh.close()
