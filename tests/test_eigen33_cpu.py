"""The plane-fit eigen solve without a GPU: tests/_eigen33_ref.py's plain fp64 twin of csrc/pcp_eigen33.hpp against
mpmath.eigsy at 50 digits over the whole case table.  What the GPU suite asks of the device (tests/test_eigen33_gpu.py) the
reference form has to meet first: every branch is run, no NaN where the eigenvector is defined, NaN where every cross
product is exactly zero, and NaN nowhere outside the exact-NaN and the ill-defined classes.  The twin's worst errors per
class -- from which the device's bars are derived at run time -- go into profiles/eigen33_selftest.md."""
import collections

import numpy as np
import pytest

import _eigen33_ref as R


@pytest.fixture(scope="module")
def table():
    return R.case_table()


@pytest.fixture(scope="module")
def done():
    return R.table_reference()


def test_table_is_seeded_and_holds_about_20000_matrices(table):
    n = len(table["mat"])
    assert 19_000 <= n <= 21_000, n
    assert np.isfinite(table["mat"]).all()
    R.case_table.cache_clear()
    again = R.case_table()
    assert np.array_equal(again["mat"].view(np.uint64), table["mat"].view(np.uint64)) and np.array_equal(again["cls"], table["cls"])
    for c in range(len(R.CLASSES)):
        assert (table["cls"] == c).sum() >= 200, R.CLASSES[c]


def test_every_branch_runs_on_at_least_100_cases(table, done):
    counts = np.bincount(done["branch"], minlength=3)
    rows = ["| branch | cases | of them per class (separated / caller-shaped / exact-NaN / ill-defined) |", "|---|---|---|"]
    for b, name in enumerate(R.BRANCHES):
        per = [int(((done["branch"] == b) & (table["cls"] == c)).sum()) for c in range(4)]
        rows.append(f"| `{name}` | {counts[b]} | {' / '.join(map(str, per))} |")
    R.write_block("branches", "\n".join(rows))
    assert (counts >= 100).all(), dict(zip(R.BRANCHES, counts.tolist()))


def test_twin_is_finite_where_the_vector_is_defined(table, done):
    defined = np.isin(table["cls"], (R.SEPARATED, R.CALLER)) & (done["gap"] >= R.GAP)
    assert defined.sum() > 10_000
    assert done["err"]["finite"][defined].all()


def test_twin_is_nan_on_every_exact_nan_case(table, done):
    sel = table["cls"] == R.EXACT_NAN
    assert np.isnan(done["vec"][sel]).all()
    assert np.isfinite(done["ev"][sel]).all()  # (the eigenvalue itself is a plain product)


def test_twin_is_nan_nowhere_else_but_in_the_ill_defined_class(table, done):
    bad = ~done["err"]["finite"] & ~np.isin(table["cls"], (R.EXACT_NAN, R.ILL))
    assert not bad.any(), collections.Counter(table["tag"][bad].tolist())
    # a vector is finite or three NaNs, never mixed, never infinite
    v = done["vec"]
    assert (np.isfinite(v).all(axis=1) | np.isnan(v).all(axis=1)).all()


def test_twin_meets_the_accuracy_the_device_is_held_to(table, done):
    """Against mpmath: the vector to 8e-16 at gap ~ 1 and 3e-11 at gap 1e-3 (error x gap stays below 3e-14 over 120 binades
    of scale), a unit vector to 4 ulp, and eigenvalue and residual at the rounding level wherever the vector is defined.  The
    worst figures per class are written into the document; the GPU suite recomputes them and multiplies by 8."""
    err, gap, w = done["err"], done["gap"], done["worst"]
    fin = err["finite"]
    assert np.nanmax(err["norm"]) <= 4 * R.U
    sel = fin & np.isin(table["cls"], (R.SEPARATED, R.CALLER)) & (gap >= R.GAP)
    assert (err["vector"][sel] * gap[sel]).max() <= 3e-14
    wide = sel & (gap >= 0.5)
    assert wide.sum() > 1000 and err["vector"][wide].max() <= 8e-16
    assert err["vector"][sel].max() <= 3e-11
    for name in ("separated", "caller-shaped"):
        assert w[name]["value"] <= 1e-12 and w[name]["residual"] <= 1e-11, (name, w[name])
    rows = ["| class | cases | finite | NaN | vector (gap >= 1e-3) | value | residual | norm |", "|---|---|---|---|---|---|---|---|"]
    for c, name in enumerate(R.CLASSES):
        m = table["cls"] == c
        rows.append(f"| {name} | {m.sum()} | {(m & fin).sum()} | {(m & ~fin).sum()} | {R.fmt(w[name]['vector'])} | "
                    f"{R.fmt(w[name]['value'])} | {R.fmt(w[name]['residual'])} | {R.fmt(w[name]['norm'])} |")
    R.write_block("twin", "\n".join(rows))
    # the families of every class, with the twin's worst residual in each (where the ill-defined class's figure comes from)
    rows = ["| class | family | cases | NaN | smallest gap | worst residual | worst value |", "|---|---|---|---|---|---|---|"]
    fam = np.array([t.split(" K=")[0].split(" at ")[0] for t in table["tag"].tolist()])
    for c, name in enumerate(R.CLASSES):
        for f in sorted(set(fam[table["cls"] == c].tolist())):
            m = (table["cls"] == c) & (fam == f)
            mf = m & fin
            rows.append(f"| {name} | {f} | {m.sum()} | {(m & ~fin).sum()} | {R.fmt(float(gap[m].min()))} | "
                        f"{R.fmt(float(err['residual'][mf].max()) if mf.any() else 0.0)} | "
                        f"{R.fmt(float(err['value'][mf].max()) if mf.any() else 0.0)} |")
    R.write_block("families", "\n".join(rows))


def test_reciprocal_reference_agrees_with_mpmath():
    """The correctly rounded 1 / x is IEEE division and 1 / sqrt(x) a long double quotient settled by mpmath near midpoints:
    both equal mpmath's rounding of the 50-digit value on a sample of the GPU suite's own arguments."""
    x = R.reciprocal_arguments()[::500]
    assert len(x) == 2000
    assert np.array_equal(R.rcp_rounded(x), R.rcp_by_mpmath(x)) and np.array_equal(R.rcp_rounded(-x), R.rcp_by_mpmath(-x))
    assert np.array_equal(R.rsqrt_rounded(x), R.rsqrt_by_mpmath(x))
    # the cases the long double cannot decide are handed to mpmath: ties of the double rounding cannot slip through
    y = R.rsqrt_rounded(np.array([4.0, 0.25, 2.0, 3.0, 2.0 ** -1000, 1.5 * 2.0 ** 999]))
    assert np.array_equal(y, R.rsqrt_by_mpmath(np.array([4.0, 0.25, 2.0, 3.0, 2.0 ** -1000, 1.5 * 2.0 ** 999])))
