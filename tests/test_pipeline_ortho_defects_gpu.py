"""The surface defects through the pipeline on a densely coloured scene ("Surface defects on ortho maps"): a wall at
3 m with one smooth dent (a cosine bump of 12 mm over a radius of 0.2 m, away from the keyframes) and a closed pier of R 0.3 seen
from outside with one dent of 12 mm towards its axis.  ortho_maps_by_facet(defects=...) must give, on the wall's planar map and
on the pier's unrolled map, a hollow at the dent's place with the dent's depth; every layer and row must be, bit for bit, what
capi.ortho_defects_host gives for the map's own depth and status layers; ortho_map(defects=...) the same on one frame given
by hand; the requests that are refused."""
import numpy as np
import pytest

import _crack_fuse_ref as cf_ref
import _crack_width_ref as cw_ref

pytestmark = pytest.mark.gpu

SHAPE = (270, 480)
GSD = 0.01
N_WALL, N_PIER = 260_000, 60_000
WALL_Z, DENT_XY, DENT_A, DENT_H = 3.0, (0.45, 0.2), 0.2, 0.012
R_PIER, PIER_AXIS, PIER_HALF_Y = 0.3, np.array([-0.7, 0.0, 2.2]), 1.0
PIER_T0 = float(np.arctan2(0.7, -2.2))  # the side of the pier that faces the keyframes
PIER_DENT_Y, PIER_DENT_ARC, PIER_DENT_HALF_Y = 0.1, 0.12, 0.15
FACET = dict(link_radius=0.05, angle_deg=10.0, plane_tol=0.01, max_curvature=0.02, min_points=1000)
REQUEST = dict(threshold=0.004, window=0, min_pixels=20)
_STATE = {}


def _bump(r):
    """1 at 0, 0 from 1 on, smooth"""
    return np.where(r < 1.0, 0.5 * (1.0 + np.cos(np.pi * np.minimum(r, 1.0))), 0.0)


def scene_points(seed=23):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1.8, 1.8, N_WALL), rng.uniform(-1.4, 1.4, N_WALL)
    z = WALL_Z + DENT_H * _bump(np.hypot(x - DENT_XY[0], y - DENT_XY[1]) / DENT_A)
    wall = np.stack([x, y, z], axis=1)
    t, y = rng.uniform(0, 2 * np.pi, N_PIER), rng.uniform(-PIER_HALF_Y, PIER_HALF_Y, N_PIER)
    dt = np.angle(np.exp(1j * (t - PIER_T0)))
    rho = R_PIER - DENT_H * _bump(np.hypot(R_PIER * dt / PIER_DENT_ARC, (y - PIER_DENT_Y) / PIER_DENT_HALF_Y))
    pier = PIER_AXIS + np.stack([rho * np.sin(t), y, rho * np.cos(t)], axis=1)
    return np.concatenate([wall, pier]).astype(np.float32)


def _run():
    if _STATE:
        return _STATE
    from pointcloudprocessor_amd import capi, pipeline, synth

    cam = cw_ref.camera(SHAPE)
    poses = cf_ref.stripe_scene()["poses"]
    pts = scene_points()
    h, w = SHAPE
    eng = pipeline.HipEngine(0)
    try:
        eng.configure(cam, capi.default_cull_params())
        eng.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
        eng.set_keyframes(poses, images=[synth.make_image(k, w, h) for k in range(len(poses))])
        col = pipeline.PointCloudColorizer(eng)
        col.run(download=False)
        before = eng.ctx.download_result_packed().copy()
        fac = col.facets(xyz=pts, normal_radius=0.05, cylinders=True, cylinder_gsd=GSD, **FACET)
        maps = col.ortho_maps_by_facet(GSD, xyz=pts, fill_radius=2, cylinders=True, defects=REQUEST)
        plain = col.ortho_maps_by_facet(GSD, xyz=pts, fill_radius=2, cylinders=True)
        frame = dict(o=(-1.8, -1.4, 0.0), u=(1, 0, 0), v=(0, 1, 0), n=(0, 0, 1), gsd=GSD, width=360, height=280, d_min=2.9, d_max=3.1)
        whole = col.ortho_map(frame=frame, fill_radius=2, defects=dict(threshold=0.004, window=25, refine=True, min_support=50, min_pixels=20))
        assert np.array_equal(eng.ctx.download_result_packed(), before), "the colour result is left alone"
    finally:
        eng.close()
    _STATE.update(pts=pts, fac=fac, maps=maps, plain=plain, whole=whole)
    return _STATE


def _map_of(s, first_point, kind):
    fac = s["fac"]
    row = int(np.flatnonzero(fac["ids"] == fac["label"][first_point])[0])
    assert fac["kind"][row] == kind, (row, fac["kind"])
    return next(m for m in s["maps"] if m["row"] == row)


def _same_as_the_twin(m, request):
    from pointcloudprocessor_amd import capi

    want = capi.ortho_defects_host(m["depth"], m["status"], **request)
    assert np.array_equal(m["defect_dev"], want["dev"]) and np.array_equal(m["defect_class"], want["cls"]) and np.array_equal(m["defect_region"], want["region"])
    assert [d["row"] for d in m["defects"]] == [[int(v) for v in r] for r in want["rows"]]
    assert [m["defect_counts"][k] for k in capi.DEFECT_OUT] == [int(v) for v in want["out"]]
    g = m["frame"]["gsd"]
    for d in m["defects"]:
        r = d["row"]
        assert d["kind"] == ("hollow" if r[0] == 1 else "bulge") and d["area_m2"] == r[1] * g * g and d["depth_m"] == r[4] * 2.0 ** -20
        assert d["volume_m3"] == r[3] * 2.0 ** -20 * g * g and d["centroid_px"] == (r[10] / r[1], r[11] / r[1])


def test_layers_and_rows_are_the_twins_and_nothing_else_changes():
    s = _run()
    assert len(s["maps"]) == len(s["plain"]) >= 2
    for m, p in zip(s["maps"], s["plain"]):
        _same_as_the_twin(m, REQUEST)
        assert all(d["facet"] == m["facet"] for d in m["defects"])
        assert not any(k.startswith("defect") for k in p)
        assert all(np.array_equal(m[k], p[k]) for k in ("index", "depth", "rgb", "status", "source")), "the map is what it is without the request"
    _same_as_the_twin(s["whole"], dict(threshold=0.004, window=25, refine=True, min_support=50, min_pixels=20))
    assert all("facet" not in d for d in s["whole"]["defects"])


def test_the_dent_of_the_wall_is_a_hollow_at_its_place():
    s = _run()
    m = _map_of(s, 0, 1)
    f = m["frame"]
    hollows = [d for d in m["defects"] if d["kind"] == "hollow"]
    print("wall:", m["depth"].shape, "occupied", m["occupied"], "filled", m["filled"], [(d["kind"], d["pixels"], round(d["depth_m"], 4)) for d in m["defects"]])
    assert m["occupied"] >= 20000 and hollows
    d = max(hollows, key=lambda d: d["pixels"])
    c, r = d["centroid_px"]
    world = np.array(f["o"]) + (c + 0.5) * f["gsd"] * np.array(f["u"]) + (r + 0.5) * f["gsd"] * np.array(f["v"])
    assert np.hypot(world[0] - DENT_XY[0], world[1] - DENT_XY[1]) < 0.03
    assert abs(d["depth_m"] - DENT_H) < 0.0015  # (the fitted plane lies within a millimetre of the wall)
    # the region is the disc where the bump exceeds the threshold: 0.5 (1 + cos(pi r / a)) >= t / h
    radius = DENT_A * np.arccos(2 * REQUEST["threshold"] / DENT_H - 1.0) / np.pi
    assert abs(d["area_m2"] - np.pi * radius ** 2) < 0.25 * np.pi * radius ** 2


def test_the_dent_of_the_pier_is_a_hollow_seen_from_outside():
    s = _run()
    m = _map_of(s, N_WALL, 2)
    hollows = [d for d in m["defects"] if d["kind"] == "hollow"]
    print("pier:", m["depth"].shape, "side", m["frame"]["side"], "occupied", m["occupied"], [(d["kind"], d["pixels"], round(d["depth_m"], 4)) for d in m["defects"]])
    assert m["frame"]["side"] == -1 and hollows
    d = max(hollows, key=lambda d: d["pixels"])
    assert abs(d["depth_m"] - DENT_H) < 0.003  # (the dent pulls the fitted radius and axis by a millimetre or two)
    assert not any(x["kind"] == "bulge" and x["pixels"] >= d["pixels"] for x in m["defects"])


def test_requests_that_are_refused():
    from pointcloudprocessor_amd import pipeline

    for bad in (dict(window=3), dict(threshold=0.002, radius=3)):
        with pytest.raises(ValueError) as e:
            pipeline.ortho_defects_request("ortho_map", bad)
        assert "defects is dict(threshold" in str(e.value)
    for call in (lambda p: p.ortho_map(defects=dict(threshold=0.002)), lambda p: p.ortho_maps_by_facet(0.01, defects=dict(threshold=0.002))):
        with pytest.raises(ValueError) as e:
            call(pipeline.PointCloudColorizer(None, rank=0, world=2))
        assert "index shard" in str(e.value)
