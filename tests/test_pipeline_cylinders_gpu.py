"""The cylindrical facets through the pipeline on a densely coloured scene ("Cylindrical facets"): a vault of R 3
seen from inside by six keyframes and a closed pier of R 0.3 seen from outside, the viewer the mean keyframe position.  A stripe
of known width painted on the vault (the keyframes' crack masks, by ray casting) goes through crack_map, the unrolled map of the
vault and ortho_crack_layers, and is met on the raster's width layer within the two pixel footprints the crack-fuse tests
allow, at the arc position it has; an L of map points on either structure reads unmirrored on the unrolled index layer: its
stem up, its foot to the viewer's right."""
import numpy as np
import pytest

import _crack_fuse_ref as cf_ref
import _crack_width_ref as cw_ref
import _ortho_cyl_ref as ref
from test_crack_fuse_gpu import _inputs

pytestmark = pytest.mark.gpu

SHAPE = (270, 480)
R_VAULT, HALF_ARC, HALF_Y = 3.0, np.radians(55.0), 1.6
R_PIER, PIER_AXIS, PIER_HALF_Y = 0.3, np.array([-0.7, 0.0, 2.2]), 1.0
W0, ARC0 = 0.05, 0.1           # the stripe: |R (theta - ARC0 / R)| < W0 / 2 on the vault, theta = atan2(x, z)
GSD = 0.005
N_VAULT, N_PIER = 280_000, 40_000
FACET = dict(link_radius=0.05, angle_deg=10.0, plane_tol=0.01, max_curvature=0.02, min_points=1000)
_STATE = {}


def scene_points(seed=17):
    rng = np.random.default_rng(seed)
    t, y = rng.uniform(-HALF_ARC, HALF_ARC, N_VAULT), rng.uniform(-HALF_Y, HALF_Y, N_VAULT)
    vault = np.stack([R_VAULT * np.sin(t), y, R_VAULT * np.cos(t)], axis=1)
    t, y = rng.uniform(0, 2 * np.pi, N_PIER), rng.uniform(-PIER_HALF_Y, PIER_HALF_Y, N_PIER)
    pier = PIER_AXIS + np.stack([R_PIER * np.sin(t), y, R_PIER * np.cos(t)], axis=1)
    return np.concatenate([vault, pier]).astype(np.float32)


def stripe_mask(cam, c2w):
    """the stripe as keyframe c2w (3 x 4) sees it: every pixel's undistorted ray through its centre, intersected with the vault
    from inside (the one positive root)"""
    h, w = SHAPE
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    x, y, ok = cw_ref.rays(cam, np.stack([2 * px.ravel(), 2 * py.ravel()], axis=1))
    m = np.asarray(c2w, np.float64).reshape(3, 4)
    d = np.stack([x, y, np.ones_like(x)], axis=1) @ m[:, :3].T
    o = m[:, 3]
    a = d[:, 0] ** 2 + d[:, 2] ** 2
    b = 2.0 * (o[0] * d[:, 0] + o[2] * d[:, 2])
    c = o[0] ** 2 + o[2] ** 2 - R_VAULT ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (-b + np.sqrt(b * b - 4.0 * a * c)) / (2.0 * a)
        p = o + s[:, None] * d
        theta = np.arctan2(p[:, 0], p[:, 2])
        fg = ok & (s > 0) & (np.abs(p[:, 1]) <= HALF_Y) & (np.abs(theta) <= HALF_ARC) & (np.abs(R_VAULT * theta - ARC0) < W0 / 2.0)
    return np.where(fg, 255, 0).astype(np.uint8).reshape(h, w)


def _run():
    """the scene through the pipeline, once: colours, the crack chain, the facets with their cylinders, the unrolled maps"""
    if _STATE:
        return _STATE
    from pointcloudprocessor_amd import capi, pipeline, synth

    cam = cw_ref.camera(SHAPE)
    poses = cf_ref.stripe_scene()["poses"]
    pts = scene_points()
    c2w = [capi.pose_to_matrices(p)[1] for p in poses]
    masks = [stripe_mask(cam, m) for m in c2w]
    assert all((m > 0).sum() > 500 for m in masks)
    h, w = SHAPE
    eng = pipeline.HipEngine(0)
    try:
        eng.configure(cam, capi.default_cull_params())
        eng.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
        eng.set_keyframes(poses, images=[synth.make_image(k, w, h) for k in range(len(poses))], masks=masks)
        col = pipeline.PointCloudColorizer(eng)
        col.run(download=False)
        has = (eng.ctx.download_result_packed() >> 24) > 0
        cracks = col.crack_map()
        inputs = _inputs(eng.ctx, range(len(poses)), 0, 150)
        fac = col.facets(xyz=pts, normal_radius=0.05, cylinders=True, cylinder_gsd=GSD, **FACET)  # (viewer: the mean keyframe position)
        maps = col.ortho_maps_by_facet(GSD, xyz=pts, cylinders=True)
        for m in maps:
            m.update(pipeline.ortho_crack_layers(m["index"], cracks["width_mean"], cracks["label"]))
    finally:
        eng.close()
    _STATE.update(cam=cam, poses=poses, pts=pts, c2w=c2w, has=has, cracks=cracks, inputs=inputs, fac=fac, maps=maps,
                  viewer=np.asarray(poses, np.float64)[:, :3].mean(axis=0))
    return _STATE


def _map_of(s, first_point):
    fac = s["fac"]
    row = int(np.flatnonzero(fac["ids"] == fac["label"][first_point])[0])
    assert fac["kind"][row] == 2, (row, fac["kind"], [None if c is None else c["stats"]["rms"] for c in fac["cylinder"]])
    return next(m for m in s["maps"] if m["row"] == row)


def test_kinds_sides_and_coverage():
    s = _run()
    fac = s["fac"]
    vault, pier = _map_of(s, 0), _map_of(s, N_VAULT)
    print("facets", fac["facets"], "kinds", fac["kind"], "coloured rows", int(s["has"][:N_VAULT].sum()), "of the vault,", int(s["has"][N_VAULT:].sum()),
          "of the pier; occupied", vault["occupied"], pier["occupied"])
    assert vault["kind"] == 2 and vault["frame"]["side"] == 1 and abs(vault["frame"]["radius"] - R_VAULT) < 2e-3
    assert pier["kind"] == 2 and pier["frame"]["side"] == -1 and abs(pier["frame"]["radius"] - R_PIER) < 1e-3
    assert pier["frame"]["width"] == int(np.ceil(2 * np.pi * pier["frame"]["radius"] / pier["frame"]["gsd"])), "the closed ring"
    assert vault["occupied"] >= 20000 and pier["occupied"] >= 2000, "the keyframes colour both structures densely"
    for m in (vault, pier):  # the depth layer is the radial deviation: these cylinders are exact
        assert np.abs(m["depth"][m["status"] == 1]).max() < 1e-3


def test_a_stripe_of_known_width_on_the_vault():
    """At the raster's pixels whose point is a crack point with centres > 0, the width layer is within two pixel footprints
    (range / fx) at the farthest credited range, divided by the smallest incidence cosine among the credited views: the bound
    of test_crack_fuse_gpu.py::test_known_stripe, with the vault's normal in the wall's place.  The stripe lies on the raster
    where it lies on the vault: its pixels' arc positions within the same bound of the painted band."""
    s = _run()
    m, cracks, pts = _map_of(s, 0), s["cracks"], s["pts"].astype(np.float64)
    far, cos_min = 0.0, 1.0
    for f, (index, pixel, rng, flags, _) in s["inputs"].items():
        ok = (flags.ravel()[pixel] & cf_ref.WIDTH) != 0
        assert ok.any(), f
        p = pts[index[ok]]
        eye = np.asarray(s["c2w"][f], np.float64).reshape(3, 4)[:, 3]
        normal = np.stack([p[:, 0], np.zeros(len(p)), p[:, 2]], axis=1) / np.hypot(p[:, 0], p[:, 2])[:, None]  # (credited rows lie on the vault)
        assert np.abs(np.hypot(p[:, 0], p[:, 2]) - R_VAULT).max() < 1e-3
        v = p - eye
        far = max(far, float(rng[ok].max()))
        cos_min = min(cos_min, float((np.abs((v * normal).sum(axis=1)) / np.linalg.norm(v, axis=1)).min()))
    bound = 2.0 * (far / s["cam"]["fx"]) / cos_min
    drawn = m["status"] == 1
    at = np.where(drawn, m["index"], 0).astype(np.int64)
    pick = drawn & (m["crack"] >= 0) & (cracks["views"][at] > 0) & (cracks["centres"][at] > 0)
    err = np.abs(m["width"][pick].astype(np.float64) - W0)
    print(f"stripe on the vault: w0 {W0 * 1e3:.1f} mm, {int(pick.sum())} centre pixels of {int((drawn & (m['crack'] >= 0)).sum())} crack pixels, "
          f"worst error {err.max() * 1e3:.3f} mm, mean {err.mean() * 1e3:.3f} mm, bound {bound * 1e3:.3f} mm (farthest range {far:.3f} m, "
          f"cos_min {cos_min:.4f})")
    assert pick.sum() > 100
    assert err.max() <= bound
    # where the stripe lies: the frame's own arc coordinate of the band's centre line, against the crack pixels' columns
    fr = m["frame"]
    centre = np.array([[R_VAULT * np.sin(ARC0 / R_VAULT), 0.0, R_VAULT * np.cos(ARC0 / R_VAULT)]], np.float32)
    _, x, _, _ = ref.coords(fr, centre)
    cols = np.nonzero(pick)[1]
    arc = (cols + 0.5) * fr["gsd"] - float(x[0]) * fr["gsd"]
    print(f"arc positions of the centre pixels about the band's centre: {arc.min() * 1e3:.2f} .. {arc.max() * 1e3:.2f} mm")
    # (a credited point lies in the painted band up to the mask's edge placement, and its pixel's centre within half a pixel of it)
    assert np.abs(arc).max() <= W0 / 2 + bound + 0.5 * fr["gsd"]
    rows = np.nonzero(pick)[0]
    # (the keyframe at the identity sees +-(H / 2) / fy of the range up and down the vault: 1.69 m of the stripe at 3 m)
    seen = 2.0 * (SHAPE[0] / 2.0 / s["cam"]["fy"]) * R_VAULT
    assert rows.max() - rows.min() > 0.9 * seen / fr["gsd"], "the stripe runs as far along the vault as the keyframes see it"


def _mark(s, m, corner, r_hat):
    """rows and columns of the L's corner, stem end and foot on the map m: the map points within 3 cm of the corner, of the
    stem (0.2 .. 0.5 m up the structure from the corner) and of the foot (0.1 .. 0.3 m to the viewer's right of it)"""
    fr = m["frame"]
    up = -np.asarray(fr["a"], np.float64)  # rows run along +a, downwards (CY6)
    look = fr["side"] * r_hat              # the viewer looks outwards from inside, inwards from outside
    assert (s["viewer"] - corner) @ look < 0, "the viewer stands on the side the frame says"
    right = np.cross(look, up)             # x right, y down, z forward: right = down x forward = look x up
    rel = s["pts"].astype(np.float64) - corner
    u, v, w = rel @ up, rel @ right, rel @ look
    near = np.abs(w) < 0.1
    sets = dict(corner=near & (np.abs(u) < 0.03) & (np.abs(v) < 0.03), stem=near & (u > 0.2) & (u < 0.5) & (np.abs(v) < 0.03),
                foot=near & (v > 0.1) & (v < 0.3) & (np.abs(u) < 0.03))
    drawn = m["status"] == 1
    at = np.where(drawn, m["index"], 0).astype(np.int64)
    out = {}
    for k, member in sets.items():
        rows, cols = np.nonzero(drawn & member[at])
        assert len(rows) >= 20, (k, len(rows), int(member.sum()))
        out[k] = (rows.mean(), cols.mean(), len(rows))
    print("side", fr["side"], {k: (round(v[0], 1), round(v[1], 1), v[2]) for k, v in out.items()})
    return out, fr["gsd"]


def _reads_unmirrored(out, gsd):
    (r0, c0, _), (r1, c1, _), (r2, c2, _) = out["corner"], out["stem"], out["foot"]
    assert abs((r0 - r1) - 0.35 / gsd) < 0.1 / gsd and abs(c1 - c0) < 0.03 / gsd, "the stem runs up the picture"
    assert 0.15 / gsd < c2 - c0 < 0.25 / gsd and abs(r2 - r0) < 0.03 / gsd, "the foot runs to the right"


def test_a_mark_on_the_vault_reads_unmirrored_from_inside():
    s = _run()
    theta = 0.35
    r_hat = np.array([np.sin(theta), 0.0, np.cos(theta)])
    _reads_unmirrored(*_mark(s, _map_of(s, 0), R_VAULT * r_hat + np.array([0.0, 0.3, 0.0]), r_hat))


def test_a_mark_on_the_pier_reads_unmirrored_from_outside():
    s = _run()
    to_viewer = s["viewer"] - PIER_AXIS
    to_viewer[1] = 0.0
    r_hat = to_viewer / np.linalg.norm(to_viewer)
    _reads_unmirrored(*_mark(s, _map_of(s, N_VAULT), PIER_AXIS + R_PIER * r_hat, r_hat))
