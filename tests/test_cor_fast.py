"""cor_fast (R/other_correlations.R) without a GPU: the front end through the numpy path (engines without cor_pairs)
against scipy and mpmath, Pearson on ill-conditioned data against exact arithmetic, the reference's own README and
testthat values, Spearman's exact p-values against permutation enumeration, the ABI constants, and the R glue of
icikt_R_cor compiled with warnings as errors."""
import ctypes
from fractions import Fraction
import math
import os
import re
import subprocess
import warnings

import mpmath
import numpy as np
import pytest
from scipy import stats

from icikendalltau_amd import _lib, api, cor_fast
from oracle.rrng import RRandom
from tests.cor_checker import assert_matches_exact, check_pairs, exact_pearson, exact_upper, ill_dense, ill_pairwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class NumpyEngine:   # no cor_pairs: the front end computes in numpy
    name = "numpy"


ENG = NumpyEngine()


def _names(k):
    return [f"s{i + 1}" for i in range(k)]


def _readme_xy():
    rr = RRandom(1234)
    rr.rnorm(1000, 100, 10)
    rr.sample(100, 50)
    rr.sample(100, 50)
    return rr.rnorm(1000), rr.rnorm(1000)


def _testthat_x():
    rr = RRandom(1234)
    return rr.rnorm(400).reshape(100, 4, order="F"), rr


def test_readme_values():
    x, y = _readme_xy()
    r5 = cor_fast(x, y, method="pearson", engine=ENG)
    rho, p = np.asarray(r5["rho"]), np.asarray(r5["pvalue"])
    assert rho[0, 1] == pytest.approx(0.00720612, abs=5e-9) and p[0, 1] == pytest.approx(0.8199608, abs=5e-8)
    assert rho[0, 0] == 1 and p[0, 0] == 0
    assert list(r5["rho"].columns) == ["x", "y"]
    m3 = np.column_stack([x, y, x])
    r6 = cor_fast(m3, colnames=["s1", "s2", "s3"], engine=ENG)
    rho, p = np.asarray(r6["rho"]), np.asarray(r6["pvalue"])
    assert np.allclose(np.diag(rho), 1) and np.all(np.diag(p) == 0)
    assert rho[0, 2] == pytest.approx(1) and p[0, 2] == 0
    assert rho[1, 2] == pytest.approx(0.00720612, abs=5e-9)


def test_testthat_other_correlations():
    x, _ = _testthat_x()
    p_res = cor_fast(x, method="pearson", colnames=_names(4), engine=ENG)
    s_res = cor_fast(x, method="spearman", colnames=_names(4), engine=ENG)
    assert np.asarray(s_res["pvalue"])[1, 0] > np.asarray(p_res["pvalue"])[1, 0]
    assert np.allclose(np.asarray(p_res["rho"]), np.corrcoef(x, rowvar=False), atol=1e-14)
    assert np.allclose(np.asarray(s_res["rho"]), stats.spearmanr(x).statistic, atol=1e-14)
    ref = stats.pearsonr(x[:, 0], x[:, 1])
    assert np.asarray(p_res["pvalue"])[1, 0] == pytest.approx(ref.pvalue, rel=1e-10)


def test_testthat_na_values():
    x, rr = _testthat_x()
    x[np.unravel_index(rr.sample(400, 40) - 1, x.shape, order="F")] = np.nan
    comp = cor_fast(x[:, 0], x[:, 1], use="complete", return_matrix=False, engine=ENG)["rho"]
    ok = ~np.isnan(x[:, 0]) & ~np.isnan(x[:, 1])
    assert comp["n_values"][0] == 84 == ok.sum()
    assert comp["rho"][0] == pytest.approx(stats.pearsonr(x[ok, 0], x[ok, 1]).statistic, abs=1e-14)
    pw1 = cor_fast(x[:, 0], x[:, 1], use="pairwise.complete.obs", return_matrix=False, engine=ENG)["rho"]
    pwa = cor_fast(x, use="pairwise.complete.obs", return_matrix=False, colnames=_names(4), engine=ENG)["rho"]
    assert pw1["rho"][0] == pwa["rho"][0]
    ok13 = ~np.isnan(x[:, 0]) & ~np.isnan(x[:, 2])
    assert pwa["rho"][1] == pytest.approx(stats.pearsonr(x[ok13, 0], x[ok13, 2]).statistic, abs=1e-14)
    ev = cor_fast(x, colnames=_names(4), return_matrix=False, engine=ENG)["rho"]
    assert np.isnan(ev["rho"]).all() and np.isnan(ev["pvalue"]).all() and np.isnan(ev["n_values"]).all()


def test_errors():
    x, _ = _testthat_x()
    with pytest.raises(ValueError, match="is not a supported"):
        cor_fast(x, use="na.or.complete", colnames=_names(4), engine=ENG)
    with pytest.raises(ValueError, match="Colnames of `x` must be be specified."):
        cor_fast(x, engine=ENG)
    with pytest.raises(ValueError, match="`x` and `y` should both be provided as vectors, or `x` should be matrix-like."):
        cor_fast(x[:, 0], engine=ENG)
    with pytest.raises(ValueError, match="Both `x` and `y` must be vectors."):
        cor_fast(x, x, engine=ENG)
    with pytest.raises(ValueError, match="'arg' should be one of 'pearson', 'spearman'"):
        cor_fast(x, method="kendall", colnames=_names(4), engine=ENG)
    with pytest.raises(ValueError, match="not enough finite observations"):
        cor_fast(x[:2], colnames=_names(4), engine=ENG)


def test_front_end_against_scipy_and_mpmath():
    rng = np.random.default_rng(7)
    X = rng.normal(size=(40, 6))
    X[:, 5] = np.round(X[:, 5])          # ties
    X[rng.random(X.shape) < 0.15] = np.nan
    names = _names(6)
    for method in ("pearson", "spearman"):
        for alt in ("two.sided", "less", "greater"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = cor_fast(X, use="pairwise.complete.obs", method=method, alternative=alt, colnames=names,
                               return_matrix=False, engine=ENG)["rho"]
            pi, pj, _ = api.setup_comparisons(names, None, diag_good=False)
            want, _w = check_pairs(X, pi, pj, method, True, alt)
            np.testing.assert_allclose(got["rho"], want[:, 0], atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(got["pvalue"], want[:, 1], atol=1e-10, rtol=1e-8, equal_nan=True)
            assert np.array_equal(got["n_values"], want[:, 2])
    mpmath.mp.dps = 50
    for n, t in ((5, 0.3), (30, 2.5), (300, -4.0), (100000, 1.7), (262142, 0.01), (50, 30.0)):
        df = n - 2
        p_mp = float(mpmath.betainc(df / 2, 0.5, 0, mpmath.mpf(df) / (df + mpmath.mpf(t) ** 2), regularized=True))
        assert api._pt(t, df, t < 0) * 2 == pytest.approx(p_mp, rel=1e-10, abs=1e-300)


@pytest.mark.parametrize("n", range(2, 10))
def test_spearman_exact_against_enumeration(n):
    for is_ in range(0, (n ** 3 - n) // 3 + 3):
        up, fact = exact_upper(n, is_)
        want_upper = 1.0 if is_ <= 0 else up / fact
        assert api._prho(is_, n, False) == pytest.approx(want_upper, abs=1e-15)
        if is_ > 0:
            assert api._prho(is_, n, True) == pytest.approx(1 - want_upper, abs=1e-15)
    rng = np.random.default_rng(n)
    x, y = rng.permutation(n).astype(float), rng.permutation(n).astype(float)
    got = cor_fast(x, y, method="spearman", engine=ENG)
    rho = stats.spearmanr(x, y).statistic
    if n > 2:
        ref = stats.permutation_test((x,), lambda a: stats.spearmanr(a, y).statistic, permutation_type="pairings",
                                     n_resamples=math.factorial(n) + 1, alternative="two-sided")
        assert np.asarray(got["rho"])[0, 1] == pytest.approx(rho, abs=1e-14)
        assert np.asarray(got["pvalue"])[0, 1] == pytest.approx(min(1.0, ref.pvalue), abs=1e-12)


def test_ties_warn_once_and_short_pairs():
    X = np.array([[1, 1, 2, 3, 4, 5], [2, 1, 3, 3, 5, 4], [np.nan, 1, 2, np.nan, np.nan, np.nan]], dtype=float).T
    with pytest.warns(RuntimeWarning, match="Cannot compute exact p-value with ties") as rec:
        got = cor_fast(X, method="spearman", use="pairwise.complete.obs", colnames=_names(3), return_matrix=False,
                       engine=ENG)["rho"]
    assert sum("ties" in str(w.message) for w in rec) == 1
    short = (np.asarray(got["s1"]) == "s3") | (np.asarray(got["s2"]) == "s3")
    assert np.isnan(got["rho"][short]).all() and (got["n_values"][short] == 2).all()   # each pair's own count


def test_abi_constants():
    src = open(os.path.join(ROOT, "include", "icikt.h")).read()
    defs = dict(re.findall(r"#define\s+(ICIKT_[A-Z0-9_]+)\s+\(?(-?\d+)u?\)?", src))
    assert int(defs["ICIKT_METHOD_PEARSON"]) == _lib.METHOD["pearson"]
    assert int(defs["ICIKT_METHOD_SPEARMAN"]) == _lib.METHOD["spearman"]
    for k, v in (("OK", _lib.COR_OK), ("SHORT", _lib.COR_SHORT), ("NA", _lib.COR_NA), ("TIES", _lib.COR_TIES)):
        assert int(defs["ICIKT_COR_" + k]) == v
    assert "icikt_cor_pairs_f64" in _lib.EXPORTS


def _fraction_rho(x, y):
    """rho of exact rationals by the two-pass definition, rounded once (an independent route to exact_pearson's)."""
    fx, fy = [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in y]
    m = len(fx)
    mx, my = sum(fx) / m, sum(fy) / m
    sxy = sum((a - mx) * (b - my) for a, b in zip(fx, fy))
    sxx = sum((a - mx) ** 2 for a in fx)
    syy = sum((b - my) ** 2 for b in fy)
    if sxx == 0 or syy == 0:
        return math.nan
    r2 = sxy * sxy / (sxx * syy)
    with mpmath.workprec(400):
        mag = mpmath.sqrt(mpmath.mpf(r2.numerator) / r2.denominator)
        return float(mag if sxy >= 0 else -mag)


def test_exact_pearson_against_fractions():
    rng = np.random.default_rng(11)
    one = np.nextafter(1.0, 2.0)
    cases = [([1.0, 2.0, 3.0], [1.0, 2.0, 3.0]), ([1.0, 2.0, 3.0], [-3.0, -4.0, -5.0]),
             ([1.0, one, 1.0, one], [0.5, 2.0, -1.0, 3.0]), ([1e300, -1e300, 5e299], [1e-300, 3e-300, -2e-300]),
             ([1e12 + 0.5, 1e12 - 0.25, 1e12 + 1.0, 1e12], [-1e6 + 1e-6, -1e6, -1e6 - 3e-6, -1e6 + 2e-6]),
             ([1e250, 0.0, 1.0, -2.0], [1.0, 2.0, 4.0, 8.0])]
    for _ in range(40):
        m = int(rng.integers(2, 9))
        sc = 10.0 ** rng.integers(-300, 301, size=2)
        off = rng.choice([0.0, 1e6, -1e12, 1e200], size=2)
        cases.append((off[0] + sc[0] * rng.normal(size=m), off[1] + sc[1] * rng.normal(size=m)))
    for x, y in cases:
        x, y = np.asarray(x, float), np.asarray(y, float)
        want = _fraction_rho(x, y)
        got = exact_pearson(x, y)
        assert (math.isnan(got) and math.isnan(want)) or got == want, (x, y, got, want)
    assert exact_pearson([1.0, 2.0, 3.0], [2.0, 4.0, 6.0]) == 1.0
    assert exact_pearson([1.0, 2.0, 3.0], [2.0, 0.0, -2.0]) == -1.0
    assert math.isnan(exact_pearson([1.0, 1.0, 1.0], [1.0, 2.0, 3.0]))
    assert math.isnan(exact_pearson([5e-324, 5e-324], [1.0, 2.0]))


def _compare_exact(X, use):
    """cor_fast through the numpy path against the exact reference (cor_checker.assert_matches_exact)."""
    names = _names(X.shape[1])
    got = cor_fast(X, use=use, colnames=names, return_matrix=False, engine=ENG)["rho"]
    pi, pj, _ = api.setup_comparisons(names, None, diag_good=False)
    want, _w = check_pairs(X, pi, pj, "pearson", use == "pairwise.complete.obs", exact=True)
    assert_matches_exact(got["rho"], got["pvalue"], got["n_values"], want, label=use)


@pytest.mark.parametrize("n", [3, 65, 2000, 65536])
def test_pearson_ill_conditioned_dense(n):
    _compare_exact(ill_dense(n, n), "everything")


@pytest.mark.parametrize("n", [3, 65, 2000, 65536])
def test_pearson_ill_conditioned_pairwise(n):
    _compare_exact(ill_pairwise(n, n + 1), "pairwise.complete.obs")
