"""The orthophoto of an unrolled map restated in numpy ("Orthophotos of unrolled maps", CT1-CT3), for
test_ortho_cyl_texture_*.py.  CT1 and CT2 operation by operation in float64 with explicit casts (numpy rounds every product and
sum on its own: no fused multiply-add); the depth behind a fine pixel is OT3's, unchanged, and everything after the point is
OT4-OT6's, both taken from _ortho_texture_ref.py."""
from unittest import mock

import numpy as np

import _ortho_texture_ref as ot

F32 = np.float32
F64 = np.float64
PI2 = F64(np.pi) / F64(2)    # the doubles nearest pi/2 and pi/4 (exact scalings of the double nearest pi)
PI4 = F64(np.pi) / F64(4)
TWO_OVER_PI = F64(float.fromhex("0x1.45f306dc9c883p-1"))  # the double nearest 2 / pi
# (-1)^j / (2j + 1)! and (-1)^j / (2j)!, j = 0..8: every factorial up to 17! is an exact double, so each is one rounded quotient
_FACT = [1]
for _n in range(1, 18):
    _FACT.append(_FACT[-1] * _n)
SIN_COEF = [F64((-1.0) ** j) / F64(_FACT[2 * j + 1]) for j in range(9)]
COS_COEF = [F64((-1.0) ** j) / F64(_FACT[2 * j]) for j in range(9)]
LAYERS, COUNTS, same, tile, depth_maps = ot.LAYERS, ot.COUNTS, ot.same, ot.tile, ot.depth_maps
_plane_surface = ot.surface  # (texture() below puts CT2's in its place for the length of a call)


def reduce(theta):
    """CT1 steps 1-2: (k, r)"""
    t = np.asarray(theta, F64)
    k = (t * TWO_OVER_PI + F64(0.5)).astype(np.int64)  # truncation, as the C cast (theta >= 0)
    return k, t - k.astype(F64) * PI2


def sincos(theta):
    """CT1: (sin, cos) of 0 <= theta < 64, operation by operation"""
    k, r = reduce(theta)
    z = r * r
    S = np.full(z.shape, SIN_COEF[8], F64)
    C = np.full(z.shape, COS_COEF[8], F64)
    for j in range(7, -1, -1):
        S = S * z + SIN_COEF[j]
        C = C * z + COS_COEF[j]
    S = r * S
    q = k & 3
    s = np.where(q == 0, S, np.where(q == 1, C, np.where(q == 2, -S, -C)))
    c = np.where(q == 0, C, np.where(q == 1, -S, np.where(q == 2, -C, S)))
    return s, c


def fine_depth(fr, source, depth, k, interpolate=True, max_step=0.05, rect=None):
    """OT3's depth behind every fine pixel, (ok, d float32): _ortho_texture_ref.surface under the frame o = 0, u = v = 0,
    n = (1, 0, 0), whose x coordinate is 0 + ((s 0 + t 0) + d 1) = d exactly (the map's depths are never -0: CY2)"""
    probe = dict(width=fr["width"], height=fr["height"], gsd=fr["gsd"], o=[0, 0, 0], u=[0, 0, 0], v=[0, 0, 0], n=[1, 0, 0])
    ok, xyz = _plane_surface(probe, source, depth, k, interpolate, max_step, rect)
    return ok, xyz[..., 0]


def surface(fr, source, depth, k, interpolate=True, max_step=0.05, rect=None):
    """CT2: (ok (h k, w k) bool, xyz (h k, w k, 3) float32, zeros where there is no surface); fr: a cylinder's frame"""
    x0, y0, w, h = ot._rect(fr, rect)
    ok, d = fine_depth(fr, source, depth, k, interpolate, max_step, rect)
    Xg, Yg = np.meshgrid(x0 * k + np.arange(w * k, dtype=np.int64), y0 * k + np.arange(h * k, dtype=np.int64))
    inv = F64(F32(F32(1.0) / F32(fr["gsd"])))
    R = F64(F32(fr["radius"]))
    xf = (Xg.astype(F64) + F64(0.5)) / F64(k)
    yf = (Yg.astype(F64) + F64(0.5)) / F64(k)
    arc, hh = xf / inv, yf / inv
    theta = arc / R
    rho = R + F64(fr["side"]) * d.astype(F64)
    ok = ok & (rho > 0)
    s, c = sincos(theta)
    rc, rs = rho * c, rho * s
    xyz = np.zeros(ok.shape + (3,), F32)
    for ax in range(3):
        cc, aa, ee, bb = (F64(F32(fr[key][ax])) for key in ("c", "a", "e", "b"))
        P = cc + ((rc * ee + rs * bb) + hh * aa)
        xyz[..., ax] = np.where(ok, P.astype(F32), F32(0))
    return ok, xyz


def texture(cam, poses, images, masks, w2cs, dmaps, fr, source, depth, k, **kw):
    """CT3: _ortho_texture_ref.texture (OT4-OT6) behind CT2's surface points; the same arguments and the same dict"""
    with mock.patch.object(ot, "surface", surface):
        return ot.texture(cam, poses, images, masks, w2cs, dmaps, fr, source, depth, k, **kw)


# -- the scenes of the tests: a vault seen from inside and a closed pier seen from outside, small rasters ---------------------
R_VAULT, HALF_ARC, HALF_Y = 3.0, np.radians(54.0), 0.76
R_PIER, PIER_AXIS, PIER_HALF_Y = 0.3, np.array([-0.7, 0.0, 2.2]), 0.35
N_VAULT, N_PIER = 120_000, 50_000
SCENE_FILL = dict(vault=2, pier=0)  # the fill radius of each map, pixels: both maps keep holes


def scene_points(seed=5):
    """the vault (R 3 about the y axis, 108 degrees of arc, waves of 1 cm and 2 mm of noise) and, between it and the keyframes,
    the pier (R 0.3, waves of 4 mm and 1 mm of noise): (n, 3) float32, the vault's rows first"""
    rng = np.random.default_rng(seed)
    t, y = rng.uniform(-HALF_ARC, HALF_ARC, N_VAULT), rng.uniform(-HALF_Y, HALF_Y, N_VAULT)
    r = R_VAULT + 0.01 * np.sin(9 * t) * np.cos(5 * y) + rng.normal(0, 0.002, N_VAULT)
    vault = np.stack([r * np.sin(t), y, r * np.cos(t)], axis=1)
    t, y = rng.uniform(0, 2 * np.pi, N_PIER), rng.uniform(-PIER_HALF_Y, PIER_HALF_Y, N_PIER)
    r = R_PIER + 0.004 * np.sin(5 * t) + rng.normal(0, 0.001, N_PIER)
    pier = PIER_AXIS + np.stack([r * np.sin(t), y, r * np.cos(t)], axis=1)
    return np.concatenate([vault, pier]).astype(np.float32)


def scene_frames():
    """dict(vault, pier) of cylinder frames: the vault an open arc of 291 x 77 pixels of 2 cm seen from inside (side +1), the
    pier a closed ring of 189 x 70 pixels of 1 cm seen from outside (side -1) whose seam faces the keyframes; b = side (a x e).
    Neither raster's sides, times 4, are a multiple of the kernel's tile of 16."""
    import _ortho_cyl_ref as cyl

    a = np.array([0.0, 1.0, 0.0])
    t0 = HALF_ARC + 0.02
    e = np.array([-np.sin(t0), 0.0, np.cos(t0)])
    vault = cyl.frame([0.0, -0.77, 0.0], a, e, np.cross(a, e), R_VAULT, 0.02, 291, 77, -0.1, 0.1, 1)
    e = np.array([0.0, 0.0, -1.0])
    pier = cyl.frame(PIER_AXIS + [0.0, -0.35, 0.0], a, e, -np.cross(a, e), R_PIER, 0.01, int(np.ceil(2 * np.pi * R_PIER / 0.01)), 70, -0.05,
                     0.05, -1)
    return dict(vault=vault, pier=pier)


def scene_poses():
    """six keyframes inside the vault, looking along +z past the pier, at different ranges and headings"""
    import _crack_fuse_ref as cf

    return np.array([[0.0, 0.0, 0.0] + cf.quaternion_y(0.0), [0.0, 0.0, 0.5] + cf.quaternion_y(0.0), [0.0, 0.0, -0.6] + cf.quaternion_y(0.0),
                     [-0.8, 0.0, 0.0] + cf.quaternion_y(15.0), [0.9, 0.1, 0.2] + cf.quaternion_y(-18.0), [0.3, -0.1, -0.3] + cf.quaternion_y(-6.0)])
