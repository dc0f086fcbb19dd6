"""The fp64 restatement of the NID histograms (tests/_nid_ref.py) pinned on the CPU before the GPU tests lean on it
(test_nid_edges_gpu.py): its cost against the C oracle and the oracle's numpy twin, its finite-difference gradient against
the oracle's dual numbers -- which is also the oracle's first finite-difference check with k3 != 0 --, and the error of
the difference quotient against the constant recorded in _nid_ref.py."""
import numpy as np
import pytest

import _nid_ref as ref
from conftest import cam_struct

CAMS = ("reference", "pincushion", "barrel")
BINS = (2, 7, 16)
T_TEST = ref.se3_exp([0.008, -0.005, 0.004, 0.004, -0.005, 0.003])  # 1 cm, 0.4 deg


@pytest.fixture(scope="module")
def inputs():
    """Two keyframes of ~1500 camera-frame points at 1 .. 2.5 m that fill a little more than the image, so that the strong
    cameras throw some out (outliers); random 8-bit images; intensities in (0, 1) with the four clamped values.  Points
    within STATUS_MARGIN_PX of a pixel boundary under any of the three cameras are left out: inputs with a margin."""
    rng = np.random.default_rng(5)
    n = 3600
    z = rng.uniform(1.0, 2.5, n)
    x, y, z = ((rng.uniform(-0.42, 0.42, n) * z).astype(np.float32), (rng.uniform(-0.24, 0.24, n) * z).astype(np.float32),
               z.astype(np.float32))
    good = np.ones(n, bool)
    for name in CAMS:
        good &= ref.status_margin(ref.camera(name), x, y, z, T_TEST) > ref.STATUS_MARGIN_PX
    x, y, z = x[good][:3000], y[good][:3000], z[good][:3000]
    assert len(x) == 3000
    inten = (0.5 + 0.45 * np.sin(3.0 * x) * np.cos(2.0 * y + 0.4)).astype(np.float32)
    inten[[3, 1503]] = 0.0
    inten[[4, 1504]] = 1.0
    inten[[5, 1505]] = -0.25
    inten[[6, 1506]] = 3.0
    images = [rng.integers(0, 256, (ref.HEIGHT, ref.WIDTH, 3), dtype=np.uint8) for _ in range(2)]
    assert all(im.min() == 0 and im.max() == 255 for im in images)
    return dict(x=x, y=y, z=z, inten=inten, images=images, off=np.array([0, 1500, 3000], np.int64))


def _rows(cd, s, bins, T=T_TEST, h=ref.H_STEP):
    o = s["off"]
    return np.stack([ref.histograms(cd, s["images"][k], s["x"][o[k]:o[k + 1]], s["y"][o[k]:o[k + 1]], s["z"][o[k]:o[k + 1]],
                                    s["inten"][o[k]:o[k + 1]], T, bins, h) for k in range(2)])


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("name", CAMS)
def test_cost_and_gradient_match_the_oracle(oracle, inputs, name, bins):
    from oracle import np_oracle

    s, cd = inputs, ref.camera(name)
    rows = _rows(cd, s, bins)
    cells = bins * bins
    for k, row in enumerate(rows):
        # the rows' own invariants: every inlier is counted once, its 16 weights sum to 1 and their derivatives to 0
        _, _, inl, _, _ = ref.project(cd, s["x"][s["off"][k]:s["off"][k + 1]], s["y"][s["off"][k]:s["off"][k + 1]],
                                      s["z"][s["off"][k]:s["off"][k + 1]], T_TEST)
        m = int(inl.sum())
        assert 1000 < m and (name == "reference" or m < 1500)  # the strong cameras have outliers
        assert row[cells * 7:].sum() == m
        assert abs(row[0:cells * 7:7].sum() - m) <= 1e-12 * m
        for c in range(1, 7):
            assert abs(row[c:cells * 7:7].sum()) <= ref.DERIV_RTOL * np.abs(row[c:cells * 7:7]).max() * cells
        # the clamped intensities land in the outer point bins
        assert row[cells * 7] >= 2 and row[cells * 7 + bins - 1] >= 2
    cost, grad, valid = ref.cost_and_gradient(rows, bins)
    c_orc, g_orc, ok = oracle.nid(cam_struct(oracle, cd), s["images"], s["off"], s["x"], s["y"], s["z"], s["inten"], T_TEST, bins)
    o = s["off"]
    c_np = sum(np_oracle.nid_cost(cd, s["images"][k], s["x"][o[k]:o[k + 1]], s["y"][o[k]:o[k + 1]], s["z"][o[k]:o[k + 1]],
                                  s["inten"][o[k]:o[k + 1]], T_TEST, bins) for k in range(2))
    assert valid and ok
    print(f"{name} bins {bins}: cost {cost!r} oracle {c_orc!r} numpy twin {c_np!r}")
    assert abs(cost - c_orc) <= 1e-12 * abs(c_orc) and abs(cost - c_np) <= 1e-12 * abs(c_np)
    bound = ref.gradient_bound(rows, bins)
    print(f"  gradient {grad} oracle {g_orc} |diff| {np.abs(grad - g_orc)} bound {bound}")
    assert np.all(np.abs(grad - g_orc) <= bound)
    assert np.abs(g_orc).max() > 1e2 * bound.max()  # ... and that bound is below a percent of the gradient itself


def test_finite_difference_error_is_within_the_recorded_bound(inputs):
    """max |D(h) - D(h/2)| per derivative plane, relative to the plane's largest magnitude: the measurement behind
    _nid_ref.FD_ERROR_MEASURED (and through it DERIV_RTOL)."""
    worst = 0.0
    for name in CAMS:
        for bins in BINS:
            a, b = _rows(ref.camera(name), inputs, bins), _rows(ref.camera(name), inputs, bins, h=ref.H_STEP / 2)
            cells = bins * bins
            for k in range(2):
                for c in range(1, 7):
                    pa, pb = a[k, c:cells * 7:7], b[k, c:cells * 7:7]
                    worst = max(worst, np.abs(pa - pb).max() / np.abs(pb).max())
    print(f"finite-difference error {worst:.3e} (recorded {ref.FD_ERROR_MEASURED:.3e})")
    assert worst <= ref.FD_ERROR_MEASURED


def test_histograms_refuse_a_point_that_crosses_a_pixel_boundary():
    cd = ref.camera("reference")
    cd.update(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
    img = np.zeros((ref.HEIGHT, ref.WIDTH, 3), np.uint8)
    z = np.float32(2.0)
    # u = cx + fx * x / z = 60 up to the rounding of x (1e-6 px), inside the step's reach of 1e-6 * fx / z = 6e-5 px
    x = np.float32((60.0 - cd["cx"]) / cd["fx"] * 2.0)
    assert ref.status_margin(cd, [x], [0.0], [z], np.eye(4))[0] < 1e-5
    with pytest.raises(AssertionError, match="changes its inlier status or its pixel"):
        ref.histograms(cd, img, [x], [0.0], [z], [0.5], np.eye(4), 4)
    row = ref.histograms(cd, img, [x + np.float32(0.01)], [0.0], [z], [0.5], np.eye(4), 4)
    assert row[4 * 4 * 7:].sum() == 1
    assert not ref.histograms(cd, img, [], [], [], [], np.eye(4), 4).any()  # no point: all zeros
    cost, grad, valid = ref.cost_and_gradient([row * 0, row], 4)  # the empty keyframe is skipped and reported
    assert not valid and cost == ref.cost_and_gradient([row], 4)[0] and np.isfinite(grad).all()
