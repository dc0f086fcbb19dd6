"""The NID stage (csrc/pcp_nid.hip) at its edges, against the fp64 restatement of its histograms (tests/_nid_ref.py, pinned
by test_nid_ref_cpu.py) and the oracle's scalars: bin counts other than 16, cameras with k3 != 0 and strong tangential terms,
the per-keyframe histograms themselves (a weight in a neighbouring cell or a derivative in the wrong slot is damped by the
entropies and can cancel across keyframes), taps clamped at every image border on a 101 x 57 image (width = 2 mod 3: the
interleaved-channel read), intensities outside [0, 1), an empty keyframe next to a one-chunk and two multi-chunk ones, the
regrow of the point buffer, images read live, and the calls that must refuse once the prepared state is stale.

The scene is not the room: one thin fronto-parallel screen of points 2 m in front of each keyframe's camera, the cameras 25 m
apart, so that the kept count of every keyframe is under control."""
import numpy as np
import pytest

import _nid_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu

SCREEN = (0, 200, 5000, 9000)  # points in front of keyframe 0 .. 3
T_IDENTITY = np.eye(4)
T_SMALL = ref.se3_exp([0.01, -0.004, 0.006, 0.002, -0.003, 0.001])
# just inside MultiNIDCost's domain (0.2 m, 2 deg): 0.19 m along and 1.9 deg about two unit vectors
T_LIMIT = ref.se3_exp(np.concatenate([0.19 * np.array([0.6, -0.64, 0.48]), np.radians(1.9) * np.array([-0.48, 0.6, 0.64])]))
EXTRINSICS = {"identity": T_IDENTITY, "small": T_SMALL, "limit": T_LIMIT}
# (camera, bins, extrinsic): every camera at 16 bins, 2 and 7 bins on the strongest camera, the three extrinsics
CASES = [("reference", 16, "small"), ("pincushion", 16, "identity"), ("pincushion", 16, "small"), ("pincushion", 16, "limit"),
         ("barrel", 16, "small"), ("barrel", 16, "limit"), ("pincushion", 2, "small"), ("pincushion", 7, "limit")]
CHUNK = 4096  # points per workgroup of k_nid_hist: a keyframe's segment is padded to a multiple


def _cull_params(module):
    cp = module.default_cull_params()
    cp.downsample_factor = 1
    return cp


def build_scene(oracle):
    """Poses, world points (fp32), intensities and images.  Candidates within STATUS_MARGIN_PX of a pixel boundary under any
    (camera, extrinsic) of CASES are left out, so that the reference's difference quotients are derivatives."""
    from pointcloudprocessor_amd import synth

    rng = np.random.default_rng(77)
    F = len(SCREEN)
    poses, _ = synth.make_trajectory(F)
    poses = poses.copy()
    poses[:, 0] += 25.0 * np.arange(F)
    any_cam, cp = cam_struct(oracle, ref.camera("reference")), _cull_params(oracle)
    xs, ys, zs, owner = [], [], [], []
    for f, want in enumerate(SCREEN):
        m = want + want // 5 + 8
        zc = rng.uniform(2.0, 2.02, m)
        pc = np.stack([rng.uniform(-0.40, 0.40, m) * zc, rng.uniform(-0.23, 0.23, m) * zc, zc], axis=1)
        w2c, c2w = oracle.pose_to_matrices(poses[f])
        M = c2w.astype(np.float64).reshape(3, 4)
        world = (pc @ M[:, :3].T + M[:, 3]).astype(np.float32)
        # the camera coordinates the stage will see: fp32 world point through the fp32 w2c
        p = oracle.project_frame(any_cam, cp, w2c, world[:, 0], world[:, 1], world[:, 2])
        good = np.ones(m, bool)
        for name, T in sorted({(c, t) for c, _, t in CASES}):
            good &= ref.status_margin(ref.camera(name), p["xc"], p["yc"], p["zc"], EXTRINSICS[T]) > ref.STATUS_MARGIN_PX
        world = world[good][:want]
        assert len(world) == want
        xs.append(world[:, 0]), ys.append(world[:, 1]), zs.append(world[:, 2]), owner.append(np.full(want, f))
    x, y, z, owner = (np.concatenate(a) for a in (xs, ys, zs, owner))
    inten = (0.5 + 0.45 * np.sin(2.1 * x) * np.sin(1.7 * y + 0.3) * np.sin(2.9 * z + 1.0)).astype(np.float32)
    assert inten.min() > 0.0 and inten.max() < 1.0
    images = [rng.integers(0, 256, (ref.HEIGHT, ref.WIDTH, 3), dtype=np.uint8) for _ in range(F)]
    assert all(im.min() == 0 and im.max() == 255 for im in images)
    return dict(poses=poses, x=x, y=y, z=z, owner=owner, inten=inten, images=images)


def clamped_intensities(oracle, s, cd):
    """The scene's intensities with exactly 0.0, exactly 1.0, -0.25 and 3.0 on four points each of every screen, chosen
    among the points nearest the image centre (kept and inliers at every extrinsic of CASES)."""
    inten = s["inten"].copy()
    cam, cp = cam_struct(oracle, cd), _cull_params(oracle)
    special = []
    for f in range(len(SCREEN)):
        idx = np.nonzero(s["owner"] == f)[0]
        if len(idx) == 0:
            continue
        w2c, _ = oracle.pose_to_matrices(s["poses"][f])
        p = oracle.project_frame(cam, cp, w2c, s["x"][idx], s["y"][idx], s["z"][idx])
        near = idx[np.argsort(np.hypot(p["xc"], p["yc"]))[:16]]
        for k, v in enumerate((0.0, 1.0, -0.25, 3.0)):
            inten[near[4 * k:4 * k + 4]] = v
        special.append(near)
    return inten, np.concatenate(special)


def culled_lists(oracle, cd, poses, x, y, z, inten):
    """Per keyframe: the oracle's culled camera-frame points with their intensity, and their indices into the cloud."""
    cam, cp = cam_struct(oracle, cd), _cull_params(oracle)
    lists = []
    for f in range(len(poses)):
        w2c, _ = oracle.pose_to_matrices(poses[f])
        keep, _, _ = oracle.cull_frame(cam, cp, w2c, x, y, z, 8)
        p = oracle.project_frame(cam, cp, w2c, x, y, z)
        sel = np.nonzero(keep)[0]
        lists.append((p["xc"][sel], p["yc"][sel], p["zc"][sel], inten[sel], sel))
    return lists


def flat(lists):
    off = np.concatenate([[0], np.cumsum([len(l[0]) for l in lists])]).astype(np.int64)
    return (off,) + tuple(np.concatenate([l[k] for l in lists]) for k in range(4))


def make_ctx(ctx, capi, cd, poses, x, y, z, inten, images):
    ctx.set_camera(cam_struct(capi, cd), _cull_params(capi))
    ctx.upload_cloud(x, y, z)
    ctx.upload_intensity(inten)
    ctx.set_frames(poses)
    for f, im in enumerate(images):
        ctx.upload_image(f, im)
    return ctx


def device_rows(ctx, F, bins):
    """The rows at pcp_nid_histograms_device, read as test_nid_over_index_shards reads them."""
    import torch

    from pointcloudprocessor_amd import pipeline

    ctx.synchronize()
    ptr, n = ctx.nid_histograms_device()
    assert n == F * (bins * bins * ref.COMP + bins)
    return torch.as_tensor(pipeline._DeviceArray(ptr, n, "<f8"), device="cuda:0").cpu().numpy().reshape(F, -1).copy()


def assert_rows_match(got, want, kept, bins, deriv_rtol=None):
    """One keyframe's row: point histogram exactly; value planes to 1e-10 * kept absolute (the worst-case fp64 summation
    error of <= 1.5e5 positive terms is ~2e-11 of their sum; a misplaced tap moves a cell by 1e-3 or more); derivative
    planes to deriv_rtol of the plane's largest magnitude (default: every cell to the value tolerance, for two GPU rows)."""
    cells = bins * bins
    assert np.array_equal(got[cells * ref.COMP:], want[cells * ref.COMP:])
    dv = np.abs(got[0:cells * ref.COMP:ref.COMP] - want[0:cells * ref.COMP:ref.COMP]).max()
    assert dv <= 1e-10 * kept, dv
    for k in range(1, ref.COMP):
        g, w = got[k:cells * ref.COMP:ref.COMP], want[k:cells * ref.COMP:ref.COMP]
        tol = 1e-10 * kept if deriv_rtol is None else deriv_rtol * np.abs(w).max()
        assert np.abs(g - w).max() <= tol, (k, np.abs(g - w).max(), tol, np.abs(w).max())


def assert_scalars_match(got, want):
    """The bars of test_nid_gpu.py: cost 1e-9 relative, gradient 1e-6 * max(|g|_inf, 1e-3)."""
    (c_got, g_got, _), (c_ref, g_ref, _) = got, want
    assert abs(c_got - c_ref) <= 1e-9 * abs(c_ref), (c_got, c_ref)
    assert np.abs(g_got - g_ref).max() <= 1e-6 * max(np.abs(g_ref).max(), 1e-3), (g_got, g_ref)


@pytest.fixture(scope="module")
def scene(oracle):
    return build_scene(oracle)


@pytest.fixture(scope="module")
def prepared(gpu_ctx_factory, oracle, scene):
    """Per camera, made once: a context that has run nid_prepare on the four keyframes, and the oracle's culled lists."""
    from pointcloudprocessor_amd import capi

    cache = {}

    def get(name):
        if name not in cache:
            cd = ref.camera(name)
            inten, special = clamped_intensities(oracle, scene, cd)
            lists = culled_lists(oracle, cd, scene["poses"], scene["x"], scene["y"], scene["z"], inten)
            # every keyframe sees its own screen only, and the clamped intensities are among its kept points
            assert all((scene["owner"][l[4]] == f).all() for f, l in enumerate(lists))
            assert np.isin(special, np.concatenate([l[4] for l in lists])).all()
            ctx = make_ctx(gpu_ctx_factory(), capi, cd, scene["poses"], scene["x"], scene["y"], scene["z"], inten, scene["images"])
            assert ctx.nid_prepare() == sum(len(l[0]) for l in lists)
            cache[name] = dict(cd=cd, ctx=ctx, lists=lists, inten=inten, special=special, images=scene["images"])
        return cache[name]

    return get


def _assert_case_conditions(p, name, T):
    """What the parity tests rely on, from the oracle's output: the keyframe shapes (none, one mostly padded chunk, two
    chunks, three chunks), the clamped point bins among the inliers, and under the strong camera taps clamped at all four
    borders and outliers."""
    kept = [len(l[0]) for l in p["lists"]]
    assert kept[0] == 0 and 0 < kept[1] < 256 and CHUNK < kept[2] <= 2 * CHUNK and 2 * CHUNK < kept[3] <= 3 * CHUNK, kept
    W, H = ref.WIDTH, ref.HEIGHT
    border = {"kx=0": 0, "kx=W-2": 0, "kx=W-1": 0, "ky=0": 0, "ky=H-2": 0, "ky=H-1": 0}
    outliers = 0
    for xc, yc, zc, inten, sel in p["lists"][1:]:
        _, _, inl, kx, ky = ref.project(p["cd"], xc, yc, zc, T)
        outliers += int((~inl).sum())
        clamped = inten[inl & np.isin(sel, p["special"])]
        assert (clamped == 0.0).sum() == 4 and (clamped == 1.0).sum() == 4 and (clamped < 0).sum() == 4 and (clamped > 1).sum() == 4
        for key, hit in (("kx=0", kx == 0), ("kx=W-2", kx == W - 2), ("kx=W-1", kx == W - 1), ("ky=0", ky == 0),
                         ("ky=H-2", ky == H - 2), ("ky=H-1", ky == H - 1)):
            border[key] += int((inl & hit).sum())
    if name == "pincushion" and T is T_IDENTITY:
        assert min(border.values()) >= 25, border
    if name == "pincushion":
        assert outliers > 0  # (at the identity too: the cull keeps u in (-1, 0), which the cost counts out)
    if T is T_LIMIT:
        assert outliers > 100
        d = np.degrees(np.arccos((np.trace(T[:3, :3]) - 1) / 2))
        assert 0.18 < np.linalg.norm(T[:3, 3]) < 0.2 and 1.8 < d < 2.0
    return kept


@pytest.mark.parametrize("name,bins,extrinsic", CASES)
def test_histograms_match_the_reference(prepared, name, bins, extrinsic):
    """Every cell of every keyframe's row at pcp_nid_histograms_device against _nid_ref.histograms.  Keyframes 1 and 2 were
    gathered before the point buffer was regrown (test_point_buffer_regrow_keeps_the_earlier_keyframes): their parity is the
    check that the device-to-device copy kept them."""
    p, T = prepared(name), EXTRINSICS[extrinsic]
    kept = _assert_case_conditions(p, name, T)
    ctx, F = p["ctx"], len(SCREEN)
    ctx.nid_accumulate(T, bins)
    rows = device_rows(ctx, F, bins)
    assert not rows[0].any()  # the keyframe without a kept point
    want = np.stack([ref.histograms(p["cd"], im, *l[:4], T, bins) for im, l in zip(p["images"], p["lists"])])
    for f in range(F):
        assert_rows_match(rows[f], want[f], max(kept[f], 1), bins, ref.DERIV_RTOL)
    # nid_finish is the entropies and the chain rule over exactly these rows
    c_fin, g_fin, ok_fin = ctx.nid_finish(bins)
    c_ref, g_ref, ok_ref = ref.cost_and_gradient(rows, bins)
    assert not ok_fin and not ok_ref
    assert abs(c_fin - c_ref) <= 1e-12 * abs(c_ref)
    np.testing.assert_allclose(g_fin, g_ref, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name,bins,extrinsic", CASES)
def test_cost_and_gradient_match_the_oracle(prepared, oracle, name, bins, extrinsic):
    """pcp_nid_evaluate against the oracle's dual numbers at the same cases.  The keyframe without points makes both sides
    report not-valid and leave it out: the cost is the sum over the other three."""
    p, T = prepared(name), EXTRINSICS[extrinsic]
    _assert_case_conditions(p, name, T)
    ctx, ocam = p["ctx"], cam_struct(oracle, p["cd"])
    want = oracle.nid(ocam, p["images"], *flat(p["lists"]), T, bins)
    got = ctx.nid_evaluate(T, bins=bins)
    assert not want[2] and not got[2]
    assert_scalars_match(got, want)
    three = oracle.nid(ocam, p["images"][1:], *flat(p["lists"][1:]), T, bins)
    assert three[2] and abs(three[0] - want[0]) <= 1e-14 * abs(want[0]) and 2.5 < three[0] <= 3.0
    assert_scalars_match(got, three)
    # inside the domain of the initial guess the same numbers come back; accumulate + finish == evaluate to rounding
    again = ctx.nid_evaluate(T, T_init=np.eye(4), bins=bins)
    ctx.nid_accumulate(T, bins)
    fin = ctx.nid_finish(bins)
    for other in (again, fin):
        assert not other[2] and abs(other[0] - got[0]) <= 1e-12 * abs(got[0])
        np.testing.assert_allclose(other[1], got[1], rtol=1e-9, atol=1e-12)


def test_optimize_refuses_a_keyframe_without_points(prepared):
    from pointcloudprocessor_amd import capi

    with pytest.raises(capi.PcpError) as e:
        prepared("pincushion")["ctx"].nid_optimize(np.eye(4))
    assert e.value.code == capi.PCP_ERR_STATE and "not finite at the initial guess" in str(e.value)


def test_point_buffer_regrow_keeps_the_earlier_keyframes(prepared, oracle, scene):
    """pcp_nid_prepare sizes its point buffer at the first keyframe that has points and regrows it, contents kept, when the
    estimate falls short.  With 4 keyframes of padded sizes [0, 4096, 8192, 12288] on a fresh context: keyframe 0 asks for
    nothing; at keyframe 1 the buffer is sized 4096 * 1.3 * 4 / 2 + 4096 = 14745 points; keyframe 2 fits (12288); keyframe 3
    needs 24576, so the buffer is regrown and the 12288 points of keyframes 1 and 2 are copied device to device.  That the
    copy kept them is what test_histograms_match_the_reference checks on this very context (rows 1 and 2).  Here: the padded
    sizes, and the same keyframes in reverse order on another fresh context -- the largest first sizes the buffer at
    12288 * 1.3 * 4 + 4096 points, no regrow -- must give the same per-keyframe histograms."""
    from pointcloudprocessor_amd import capi

    p = prepared("pincushion")
    kept = np.array([len(l[0]) for l in p["lists"]])
    padded = -(-kept // CHUNK) * CHUNK
    assert padded.tolist() == [0, 4096, 8192, 12288]
    assert int(4096 * 1.3 * 4 / 2) + 4096 == 14745 and padded[:3].sum() <= 14745 < padded.sum()
    F, bins = len(SCREEN), 16
    p["ctx"].nid_accumulate(T_SMALL, bins)
    forward = device_rows(p["ctx"], F, bins)
    with capi.Context(0) as ctx:
        make_ctx(ctx, capi, p["cd"], scene["poses"][::-1], scene["x"], scene["y"], scene["z"], p["inten"], p["images"][::-1])
        assert ctx.nid_prepare() == kept.sum()
        ctx.nid_accumulate(T_SMALL, bins)
        backward = device_rows(ctx, F, bins)
    for f in range(F):
        assert_rows_match(backward[F - 1 - f], forward[f], max(kept[f], 1), bins)


def test_images_are_read_at_every_evaluation(oracle, scene):
    """An image uploaded after pcp_nid_prepare is the one the next evaluation bins: no error, the oracle's numbers."""
    from pointcloudprocessor_amd import capi

    cd = ref.camera("barrel")
    sel = scene["owner"] > 0  # keyframes 1 .. 3: every keyframe has points, the cost is valid
    x, y, z, inten, poses = scene["x"][sel], scene["y"][sel], scene["z"][sel], scene["inten"][sel], scene["poses"][1:]
    images = list(scene["images"][1:])
    lists = culled_lists(oracle, cd, poses, x, y, z, inten)
    ocam = cam_struct(oracle, cd)
    with capi.Context(0) as ctx:
        make_ctx(ctx, capi, cd, poses, x, y, z, inten, images)
        assert ctx.nid_prepare() == sum(len(l[0]) for l in lists)
        before = ctx.nid_evaluate(T_SMALL)
        want = oracle.nid(ocam, images, *flat(lists), T_SMALL)
        assert before[2] and want[2]
        assert_scalars_match(before, want)
        images[1] = np.ascontiguousarray(255 - images[1][::-1, ::-1])
        ctx.upload_image(1, images[1])
        after = ctx.nid_evaluate(T_SMALL)
        want = oracle.nid(ocam, images, *flat(lists), T_SMALL)
        assert after[2] and want[2] and abs(after[0] - before[0]) > 1e-6
        assert_scalars_match(after, want)


def test_argument_and_order_errors(prepared):
    from pointcloudprocessor_amd import capi

    ctx = prepared("reference")["ctx"]

    def evaluator(T, bins):
        raise AssertionError("the evaluator must not be reached")

    for bins in (1, 17):
        for call in (lambda: ctx.nid_evaluate(T_SMALL, bins=bins), lambda: ctx.nid_accumulate(T_SMALL, bins),
                     lambda: ctx.nid_optimize(T_SMALL, bins=bins), lambda: ctx.nid_optimize_with(evaluator, T_SMALL, bins=bins)):
            with pytest.raises(capi.PcpError) as e:
                call()
            assert e.value.code == capi.PCP_ERR_INVALID
    ctx.nid_accumulate(T_SMALL, 16)
    with pytest.raises(capi.PcpError) as e:
        ctx.nid_finish(7)
    assert e.value.code == capi.PCP_ERR_STATE
    ctx.nid_finish(16)


@pytest.mark.parametrize("change", ["frames", "camera", "cloud"])
def test_stale_prepared_state_is_refused(oracle, scene, change):
    """pcp_nid_prepare gathers the culled points in the camera frames of the keyframes, through the camera, from the cloud
    and its intensities: after pcp_set_frames (other poses, same count), pcp_set_camera (another focal length) or a new
    pcp_upload_cloud + pcp_upload_intensity every evaluation call must refuse with PCP_ERR_STATE instead of evaluating the
    points of the old inputs (or, after an upload, no points at all with PCP_OK), until pcp_nid_prepare has run again --
    and then the numbers are the oracle's for the new inputs.

    Before nid_release() existed, on this scene: after set_frames pcp_nid_evaluate returned PCP_OK with the old poses' cost
    2.97340598 (2.97278277 once prepared again) and pcp_nid_optimize walked 21 evaluations on the old points; after
    set_camera PCP_OK with the old points through the new focal length; after the uploads PCP_OK, cost 0, valid 0."""
    from pointcloudprocessor_amd import capi

    cd = ref.camera("reference")
    sel = scene["owner"] > 0  # keyframes 1 .. 3: the cost is finite, so nid_optimize has no other reason to refuse
    x, y, z, inten, poses = scene["x"][sel], scene["y"][sel], scene["z"][sel], scene["inten"][sel], scene["poses"][1:]
    images = scene["images"][1:]
    with capi.Context(0) as ctx:
        make_ctx(ctx, capi, cd, poses, x, y, z, inten, images)
        lists = culled_lists(oracle, cd, poses, x, y, z, inten)
        assert ctx.nid_prepare() == sum(len(l[0]) for l in lists)
        first = ctx.nid_evaluate(T_SMALL)
        want = oracle.nid(cam_struct(oracle, cd), images, *flat(lists), T_SMALL)
        assert first[2] and want[2]
        assert_scalars_match(first, want)
        if change == "frames":
            poses = poses.copy()
            poses[:, :3] += [0.03, -0.02, 0.01]
            ctx.set_frames(poses)
        elif change == "camera":
            cd = dict(cd, fx=cd["fx"] * 0.9, fy=cd["fy"] * 0.9)
            ctx.set_camera(cam_struct(capi, cd), _cull_params(capi))
        else:
            x, y, z, inten = x[::2], y[::2], z[::2], inten[::2]
            ctx.upload_cloud(x, y, z)
            ctx.upload_intensity(inten)
        for call in (lambda: ctx.nid_evaluate(T_SMALL), lambda: ctx.nid_accumulate(T_SMALL, 16), lambda: ctx.nid_optimize(T_SMALL),
                     lambda: ctx.nid_finish(16), lambda: ctx.nid_histograms_device()):
            with pytest.raises(capi.PcpError) as e:
                call()
            assert e.value.code == capi.PCP_ERR_STATE, str(e.value)
        if change != "cloud":  # the images belong to the keyframe set and are sized by the camera: both calls drop them
            for f, im in enumerate(images):
                ctx.upload_image(f, im)
        lists = culled_lists(oracle, cd, poses, x, y, z, inten)
        assert ctx.nid_prepare() == sum(len(l[0]) for l in lists)
        second = ctx.nid_evaluate(T_SMALL)
        want = oracle.nid(cam_struct(oracle, cd), images, *flat(lists), T_SMALL)
        assert second[2] and want[2] and abs(want[0] - first[0]) > 1e-6  # the new inputs give another cost
        assert_scalars_match(second, want)
        _, cost, evals = ctx.nid_optimize(T_SMALL, max_outer_iterations=1)
        assert evals >= 1 and np.isfinite(cost)
