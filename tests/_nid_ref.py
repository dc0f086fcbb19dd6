"""Restatement of the NID stage's per-keyframe joint histograms (NIDCost::operator(), nid_cost.hpp:42-116) in numpy, fp64:
what the rows at pcp_nid_histograms_device are compared against.  Independent of csrc/pcp_nid.hip and of
oracle/pcp_oracle_nid.c: the value planes and the point histogram are the definition written out, and the six
SE(3)-tangent derivative planes are central differences of the value planes along T * exp(+-h e_k) -- no analytic
Jacobian of the projection, of the spline or of the group action appears here.  Only the pinhole + plumb-bob model itself
is shared (oracle.np_oracle.project).

Row layout (the device's): cell (bin_image * bins + bin_points) * 7 + 0 = value, + 1 .. + 6 = d/d(upsilon, omega), then
`bins` entries of the point histogram."""
import numpy as np

from oracle import np_oracle

COMP = 7  # value + 6 tangent derivatives

# Step of the central differences.
H_STEP = 1e-6
# Error of the difference quotient, measured on the CPU against this file alone (test_nid_ref_cpu.py::
# test_finite_difference_error_is_within_the_recorded_bound prints it and checks that it has not grown): max over the
# three cameras and bins in {2, 7, 16} of  max |D(h) - D(h/2)| / max |D(h/2)|  per derivative plane of a keyframe, on the
# 101 x 57 inputs of that test (fx ~ 119) at a 1 cm / 0.4 deg extrinsic:  2.246e-08, recorded rounded up.  It is the
# truncation term h^2 B''' (du/d delta)^3 / 6 relative to B' du/d delta, (h du/d delta)^2 ~ (1e-6 * 140)^2 = 2e-8 times a
# factor of order 1; the rounding of the per-tap weight differences over 2h is an order below it.
FD_ERROR_MEASURED = 2.3e-08
# Tolerance of every comparison against a derivative plane, relative to the plane's largest magnitude, on the CPU and on
# the GPU: ten times the measurement (one run on one input: the factor covers other inputs and extrinsics) plus 1e-9.
DERIV_RTOL = 10.0 * FD_ERROR_MEASURED + 1e-9
# Points whose u or v lies closer than this to an integer are kept out of the inputs: the finite-difference steps move a
# pixel coordinate by h * |du/d delta| <= 1e-6 * fx * (1 + r^2) * (1 + |p|) ~ 6e-4 px at fx ~ 119 and |p| < 2.5 m.
STATUS_MARGIN_PX = 2e-3


# The cameras of the NID edge tests: the reference's distortion and the two strong models of tests/test_pretest_gpu.py (the
# only ones in the suite with k3 != 0 and tangential terms above 1e-3).
DISTORTIONS = {
    "reference": {},
    "pincushion": dict(k1=0.35, k2=0.4, p1=-0.01, p2=0.02, k3=0.2),
    "barrel": dict(k1=-0.28, k2=0.07, p1=0.0012, p2=-0.0009, k3=-0.004),
}
WIDTH, HEIGHT = 101, 57  # both odd, the width = 2 mod 3 (the interleaved-channel read), no multiple of anything


def camera(name):
    """synth's "tiny" camera scaled to 101 x 57 (fx = fy ~ 118.8, centre at the image centre) with the named distortion."""
    from pointcloudprocessor_amd import synth

    cd = synth.camera_dict("tiny")
    s = WIDTH / 480.0
    cd.update(fx=cd["fx"] * s, fy=cd["fy"] * s, cx=cd["cx"] * s, cy=cd["cy"] * s)
    cd.update(image_width=WIDTH, image_height=HEIGHT, cull_width=WIDTH, cull_height=HEIGHT)
    cd.update(DISTORTIONS[name])
    return cd


def se3_exp(d):
    """Sophus SE3::exp of delta = (upsilon, omega) as a 4x4 matrix."""
    d = np.asarray(d, np.float64)
    up, om = d[:3], d[3:]
    th = np.linalg.norm(om)
    K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    if th < 1e-5:  # series: the closed forms cancel badly for the steps of the difference quotient
        A, B, Cc = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        A, B, Cc = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + A * K + B * (K @ K)
    M[:3, 3] = (np.eye(3) + B * K + Cc * (K @ K)) @ up
    return M


def project(cam, xc, yc, zc, T):
    """Pixel coordinates (u, v) of T * p, the inlier mask of nid_cost.hpp:66-69 and floor(u), floor(v)."""
    P = np.stack([np.asarray(a, np.float32).astype(np.float64) for a in (xc, yc, zc)], axis=1)
    T = np.asarray(T, np.float64).reshape(4, 4)
    pc = P @ T[:3, :3].T + T[:3, 3]
    u, v = np_oracle.project(cam, pc[:, 0], pc[:, 1], pc[:, 2])
    fin = np.isfinite(u) & np.isfinite(v) & (np.abs(u) <= 1e9) & (np.abs(v) <= 1e9)
    kx = np.floor(np.where(fin, u, -1.0)).astype(np.int64)
    ky = np.floor(np.where(fin, v, -1.0)).astype(np.int64)
    inl = fin & (kx >= 0) & (ky >= 0) & (kx < cam["image_width"]) & (ky < cam["image_height"])
    return u, v, inl, kx, ky


def status_margin(cam, xc, yc, zc, T):
    """Per point: the distance in pixels of u and v from the nearest integer (the smaller of the two), i.e. how far the
    point is from changing floor(u), floor(v) or its inlier status.  Points that are not finite report 0."""
    u, v, _, _, _ = project(cam, xc, yc, zc, T)
    with np.errstate(invalid="ignore"):
        m = np.minimum(np.abs(u - np.round(u)), np.abs(v - np.round(v)))
    return np.where(np.isfinite(m), m, 0.0)


def _weights(s):
    """The uniform cubic B-spline's four weights at offset s in [0, 1) (taps k-1 .. k+2), shape (4, m)."""
    t = 1.0 - s
    return np.stack([t * t * t, 3.0 * s * s * s - 6.0 * s * s + 4.0, 3.0 * t * t * t - 6.0 * t * t + 4.0, s * s * s]) / 6.0


def _tap_bins(cam, image, kx, ky, bins):
    """Image bin of each of the 4 x 4 taps around (kx, ky): taps clamped to the image, the image read as the reference
    reads it -- element x of the interleaved row, channel x % 3 of pixel x / 3 -- and min(int(pix * bins), bins - 1).
    Shape (4, 4, m), first axis = tap in x."""
    W, H = cam["image_width"], cam["image_height"]
    img = np.asarray(image, np.uint8).reshape(H, W, 3)
    out = np.empty((4, 4, len(kx)), np.int64)
    for a in range(4):
        px = np.clip(kx - 1 + a, 0, W - 1)
        for b in range(4):
            py = np.clip(ky - 1 + b, 0, H - 1)
            pix = img[py, px // 3, px % 3].astype(np.float64) / 255.0
            out[a, b] = np.minimum((pix * bins).astype(np.int64), bins - 1)
    return out


def _point_bins(intensity, bins):
    b = (np.asarray(intensity, np.float32).astype(np.float64) * bins).astype(np.int64)  # truncation, as the cast to int
    return np.clip(b, 0, bins - 1)


def histograms(cam, image, xc, yc, zc, intensity, T, bins, h=H_STEP):
    """One keyframe's row in the device layout (bins * bins * 7 + bins doubles) at T = T_camera_lidar.

    Derivative planes: the difference quotient of the value planes, taken tap by tap -- (w(+h) - w(-h)) / 2h summed
    into the tap's cell, which is the central difference of the planes because a point keeps its taps: the function
    ASSERTS that no point changes its inlier status or its floor(u), floor(v) between -h, 0 and +h (otherwise the
    quotient is no derivative).  Differencing before summing keeps the rounding of the large cells out of it."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    cells = bins * bins
    row = np.zeros(cells * COMP + bins)
    if len(xc) == 0:
        return row
    u, v, inl, kx, ky = project(cam, xc, yc, zc, T)
    bp = _point_bins(intensity, bins)[inl]
    row[cells * COMP:] = np.bincount(bp, minlength=bins)  # outliers are skipped before the point count
    kxi, kyi = kx[inl], ky[inl]
    cell = _tap_bins(cam, image, kxi, kyi, bins) * bins + bp  # (4, 4, m)

    def tap_weights(uu, vv):
        wu, wv = _weights(uu[inl] - kxi), _weights(vv[inl] - kyi)
        return wu[:, None, :] * wv[None, :, :]  # (4, 4, m)

    row[0:cells * COMP:COMP] = np.bincount(cell.ravel(), weights=tap_weights(u, v).ravel(), minlength=cells)
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        up, vp, inl_p, kx_p, ky_p = project(cam, xc, yc, zc, T @ se3_exp(e))
        um, vm, inl_m, kx_m, ky_m = project(cam, xc, yc, zc, T @ se3_exp(-e))
        same = np.array_equal(inl_p, inl) and np.array_equal(inl_m, inl)
        same = same and all(np.array_equal(a[inl], b) for a, b in ((kx_p, kxi), (kx_m, kxi), (ky_p, kyi), (ky_m, kyi)))
        assert same, f"a point changes its inlier status or its pixel within +-{h} along tangent direction {k}"
        dw = (tap_weights(up, vp) - tap_weights(um, vm)) / (2.0 * h)
        row[1 + k:cells * COMP:COMP] = np.bincount(cell.ravel(), weights=dw.ravel(), minlength=cells)
    return row


def nid_of_row(row, bins):
    """One keyframe: (NID, c) with c[bin_image, bin_points] = d NID / d (value of that cell), at a fixed point count --
    the gradient is linear in the derivative planes, g_k = sum(c * D_k).  NID = (H_ip - MI) / H_ip with
    MI = H_i + H_p - H_ip, i.e. 2 - (H_i + H_p) / H_ip; entropies as -sum p log(p + 1e-6) (nid_cost.hpp:95-108).
    (nan, None) for a keyframe without inliers (its point histogram sums to 0)."""
    cells = bins * bins
    row = np.asarray(row, np.float64)
    n = row[cells * COMP:].sum()
    if n == 0:
        return np.nan, None
    joint = row[0:cells * COMP:COMP].reshape(bins, bins) / n
    marg = joint.sum(axis=1)  # the image histogram
    p_pts = row[cells * COMP:] / n

    def entropy(p):
        return -(p * np.log(p + 1e-6)).sum()

    def dentropy(p):  # -dH/dp
        return np.log(p + 1e-6) + p / (p + 1e-6)

    H_ip, H_i, H_p = entropy(joint), entropy(marg), entropy(p_pts)
    with np.errstate(all="ignore"):
        nid = 2.0 - (H_i + H_p) / H_ip
        c = (dentropy(marg)[:, None] / H_ip - (H_i + H_p) * dentropy(joint) / H_ip ** 2) / n
    return nid, c


def cost_and_gradient(rows, bins):
    """(cost, gradient (6,), valid) from the keyframes' rows, summed as MultiNIDCost sums; a keyframe whose NID is not
    finite is left out and valid is False, as the library's nid_finish does."""
    cells = bins * bins
    cost, grad, valid = 0.0, np.zeros(6), True
    for row in np.asarray(rows, np.float64).reshape(-1, cells * COMP + bins):
        nid, c = nid_of_row(row, bins)
        if not np.isfinite(nid):
            valid = False
            continue
        cost += nid
        grad += np.array([(c.ravel() * row[1 + k:cells * COMP:COMP]).sum() for k in range(6)])
    return cost, grad, valid


def gradient_bound(rows, bins, rtol=DERIV_RTOL):
    """What an error of rtol * max |D_k| in every cell of every derivative plane can do to the gradient: per component
    k, sum over the keyframes of  rtol * max |D_k| * sum |c|."""
    cells = bins * bins
    out = np.zeros(6)
    for row in np.asarray(rows, np.float64).reshape(-1, cells * COMP + bins):
        nid, c = nid_of_row(row, bins)
        if np.isfinite(nid):
            out += np.array([rtol * np.abs(row[1 + k:cells * COMP:COMP]).max() * np.abs(c).sum() for k in range(6)])
    return out
