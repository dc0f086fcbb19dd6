"""The device's plane-fit eigen solve on its own (pcp_selftest_eigen33: smallest_eigenpair, mls_rcp and mls_rsqrt of
csrc/pcp_eigen33.hpp as the units compile them) against mpmath at 50 digits, in both forms: 0 = without contraction (map
normals; also how the crack-width and crack-direction units are built), 1 = with (the MLS fit).

The bars come from tests/_eigen33_ref.py at run time: 8 x the worst error of the plain fp64 twin against the same reference in
the same class, with a floor of 16 x 2^-53 -- the device differs from the twin by its 1-2 ulp reciprocals, by another libm
(atan2, cos, sin, sqrt) and, in form 1, by fused products, each worth a few ulp of an intermediate.  Never from the device's
own output.  tests/test_eigen33_cpu.py shows that the twin itself keeps every rule asked of the device here."""
import collections

import numpy as np
import pytest

import _eigen33_ref as R

pytestmark = pytest.mark.gpu

FORMS = (0, 1)


@pytest.fixture(scope="module")
def table():
    return R.case_table()


@pytest.fixture(scope="module")
def done():
    return R.table_reference()


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()  # no camera, no cloud


@pytest.fixture(scope="module")
def device(ctx, table, done):
    """Per form: the device's (ev, vec) over the table and their errors against the reference; computed once."""
    out = {}
    for form in FORMS:
        ev, vec, _, _ = ctx.selftest_eigen33(form, table["mat"])
        out[form] = dict(ev=ev, vec=vec, err=R.errors(table["mat"], ev, vec, done["ref"]))
    return out


def _bar(twin_worst):
    return max(R.MARGIN * twin_worst, R.FLOOR)


@pytest.mark.parametrize("form", FORMS)
def test_every_finite_result_is_a_unit_eigenpair_to_the_twins_accuracy(table, done, device, form):
    err = device[form]["err"]
    worst = R.worst(err, table["cls"], done["gap"])
    rows = ["| class | finite | NaN | vector (gap >= 1e-3) | ratio | value | ratio | residual | ratio | norm |", "|---|---|---|---|---|---|---|---|---|---|"]
    for c, name in enumerate(R.CLASSES):
        m = table["cls"] == c
        tw, dv = done["worst"][name], worst[name]
        ratio = {k: (f"{dv[k] / tw[k]:.2f}" if tw[k] * R.MARGIN > R.FLOOR else "-") for k in ("vector", "value", "residual")}
        rows.append(f"| {name} | {(m & err['finite']).sum()} | {(m & ~err['finite']).sum()} | {R.fmt(dv['vector'])} | {ratio['vector']} | "
                    f"{R.fmt(dv['value'])} | {ratio['value']} | {R.fmt(dv['residual'])} | {ratio['residual']} | {R.fmt(dv['norm'])} |")
    print(f"\nform {form}\n" + "\n".join(rows))
    R.write_block(f"device form {form}", "\n".join(rows))
    fin = err["finite"]
    assert np.nanmax(err["norm"]) <= R.FLOOR, np.nanmax(err["norm"])
    for c, name in enumerate(R.CLASSES):
        sel = fin & (table["cls"] == c)
        if not sel.any():
            continue
        for k in ("residual", "value"):
            bar = _bar(done["worst"][name][k])
            over = sel & (err[k] > bar)
            assert not over.any(), (form, name, k, float(err[k][sel].max()), bar, collections.Counter(table["tag"][over].tolist()).most_common(5))


@pytest.mark.parametrize("form", FORMS)
def test_defined_eigenvectors_are_finite_and_as_close_as_the_twins(table, done, device, form):
    err = device[form]["err"]
    for c in (R.SEPARATED, R.CALLER):
        sel = (table["cls"] == c) & (done["gap"] >= R.GAP)
        assert sel.sum() > 3000
        assert err["finite"][sel].all(), (form, R.CLASSES[c], collections.Counter(table["tag"][sel & ~err["finite"]].tolist()))
        bar = R.MARGIN * done["worst"][R.CLASSES[c]]["vector"]
        assert bar > 0
        over = sel & (err["vector"] > bar)
        assert not over.any(), (form, R.CLASSES[c], float(err["vector"][sel].max()), bar, collections.Counter(table["tag"][over].tolist()).most_common(5))


@pytest.mark.parametrize("form", FORMS)
def test_exact_nan_cases_are_three_nans(table, device, form):
    sel = table["cls"] == R.EXACT_NAN
    assert sel.sum() > 200
    assert np.isnan(device[form]["vec"][sel]).all()


@pytest.mark.parametrize("form", FORMS)
def test_results_are_non_finite_only_where_the_vector_is_undefined(table, device, form):
    """The cap: NaN in the exact-NaN class, NaN or a unit eigenpair in the ill-defined one (the rules of the first test),
    finite everywhere else; a vector is three NaNs or three finite numbers, the eigenvalue always finite."""
    vec, ev = device[form]["vec"], device[form]["ev"]
    fin = np.isfinite(vec).all(axis=1)
    assert (fin | np.isnan(vec).all(axis=1)).all()
    assert np.isfinite(ev).all()
    bad = ~fin & ~np.isin(table["cls"], (R.EXACT_NAN, R.ILL))
    assert not bad.any(), (form, collections.Counter(table["tag"][bad].tolist()))
    assert fin[table["cls"] == R.ILL].any() and (~fin[table["cls"] == R.ILL]).any()  # both outcomes occur, both are right


@pytest.fixture(scope="module")
def reciprocal_case():
    x = R.reciprocal_arguments()
    neg = -x[::2]
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
    args = np.concatenate([x, neg, special])
    return dict(args=args, n_pos=len(x), n_neg=len(neg), rcp=R.rcp_rounded(args[:len(x) + len(neg)]), rsqrt=R.rsqrt_rounded(x))


@pytest.mark.parametrize("form", FORMS)
def test_reciprocals_are_within_two_ulp_of_the_correctly_rounded_value(ctx, reciprocal_case, form):
    """mls_rcp and mls_rsqrt on 2^k (1 + f), k in [-1000, 1000]: the header's own claim, "an ulp or two", against the
    correctly rounded 1 / x and 1 / sqrt(x); and the non-finite results the callers' guards rely on."""
    rc = reciprocal_case
    _, _, rcp, rsq = ctx.selftest_eigen33(form, None, rc["args"])
    n, k = rc["n_pos"], rc["n_neg"]
    u_rcp = R.ulps(rcp[:n + k], rc["rcp"])
    u_rsq = R.ulps(rsq[:n], rc["rsqrt"])
    rows = ["| function | arguments | worst | share above 1 ulp | share exact |", "|---|---|---|---|---|",
            f"| `mls_rcp` | {n + k} | {u_rcp.max():.3f} | {(u_rcp > 1).mean():.2e} | {(u_rcp == 0).mean():.4f} |",
            f"| `mls_rsqrt` | {n} | {u_rsq.max():.3f} | {(u_rsq > 1).mean():.2e} | {(u_rsq == 0).mean():.4f} |"]
    print(f"\nform {form}\n" + "\n".join(rows))
    R.write_block(f"reciprocals form {form}", "\n".join(rows))
    assert u_rcp.max() <= 2.0, (u_rcp.max(), rc["args"][np.argmax(u_rcp)])
    assert u_rsq.max() <= 2.0, (u_rsq.max(), rc["args"][np.argmax(u_rsq)])
    assert np.array_equal(np.signbit(rcp[:n + k]), np.signbit(rc["args"][:n + k]))
    assert not np.isfinite(rsq[n:n + k]).any()  # negative arguments of the root
    assert not np.isfinite(rcp[n + k:]).any() and not np.isfinite(rsq[n + k:]).any()  # 0, -0, inf, -inf, NaN


def test_refusals_and_empty_calls(ctx):
    from pointcloudprocessor_amd import capi
    import ctypes as C

    lib, h = ctx.lib, ctx.h
    one = np.zeros(6)
    out = np.zeros(3)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda form, n, mat, ev, vec, m, arg, rcp, rsq: lib.pcp_selftest_eigen33(  # noqa: E731
        h, C.c_int32(form), C.c_int64(n), mat, ev, vec, C.c_int64(m), arg, rcp, rsq)
    assert call(0, 0, None, None, None, 0, None, None, None) == capi.PCP_OK
    assert call(1, 0, None, None, None, 0, None, None, None) == capi.PCP_OK
    for bad in (lambda: call(2, 0, None, None, None, 0, None, None, None), lambda: call(-1, 0, None, None, None, 0, None, None, None),
                lambda: call(0, -1, p(one), p(out), p(out), 0, None, None, None), lambda: call(0, 0, None, None, None, -1, p(one), p(out), p(out)),
                lambda: call(0, 1, None, p(out), p(out), 0, None, None, None), lambda: call(0, 1, p(one), None, p(out), 0, None, None, None),
                lambda: call(1, 1, p(one), p(out), None, 0, None, None, None), lambda: call(1, 0, None, None, None, 1, None, p(out), p(out)),
                lambda: call(1, 0, None, None, None, 1, p(one), None, p(out)), lambda: call(0, 0, None, None, None, 1, p(one), p(out), None),
                lambda: call(0, (1 << 27) + 1, p(one), p(out), p(out), 0, None, None, None)):
        assert bad() == capi.PCP_ERR_INVALID
    assert lib.pcp_selftest_eigen33(None, C.c_int32(0), C.c_int64(0), None, None, None, C.c_int64(0), None, None, None) == capi.PCP_ERR_INVALID
    ev, vec, rcp, rsq = ctx.selftest_eigen33(0)
    assert len(ev) == len(rcp) == 0
    # one matrix, one argument, known answers: diag(3, 2, 1) -> 1 and +-z; 4 -> 1/4 and 1/2
    ev, vec, rcp, rsq = ctx.selftest_eigen33(1, [[3.0, 0, 0, 2.0, 0, 1.0]], [4.0])
    assert abs(ev[0] - 1.0) <= 1e-15 and abs(abs(vec[0, 2]) - 1.0) <= 1e-15 and np.abs(vec[0, :2]).max() <= 1e-15
    assert rcp[0] == 0.25 and rsq[0] == 0.5


def test_no_state_of_the_context_changes(gpu_ctx_factory):
    """A normals estimate and an MLS result fetched before and after both forms of the self-test are the same bytes, and the
    timers of the stages do not move."""
    from pointcloudprocessor_amd import capi

    rng = np.random.default_rng(3)
    pts = (rng.uniform(-0.1, 0.1, (3000, 3)) * [1, 1, 0.02] + [2.0, -1.0, 0.5]).astype(np.float32)
    c = gpu_ctx_factory()
    c.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
    valid = c.estimate_normals(0.03)
    mp = capi.default_mls_params()
    mp.upsampling = 0
    rows = c.mls_process(mp)
    assert valid > 0 and rows > 0
    n0, m0 = c.normals_fetch(), c.mls_fetch(rows)
    mat = R.case_table()["mat"][::37]
    for form in FORMS:
        ev, vec, rcp, rsq = c.selftest_eigen33(form, mat, [2.0, 3.0])
        assert len(ev) == len(mat) and np.isfinite(rcp).all()
    n1, m1 = c.normals_fetch(), c.mls_fetch(rows)
    for k in n0:
        assert np.array_equal(n0[k].view(np.uint32), n1[k].view(np.uint32)), k
    for k in m0:
        assert m0[k].tobytes() == m1[k].tobytes(), k
    assert c.estimate_normals(0.03) == valid and c.mls_process(mp) == rows
