"""cor_fast on the MI355X (icikt_cor_pairs_f64) against the CPU checker (tests/cor_checker.py): rho |d| <= 1e-12,
p |d| <= 1e-10 and <= 1e-8 relative where p >= 1e-290, n_values exact."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api, cor_fast
from tests.cor_checker import check_pairs

pytestmark = pytest.mark.gpu


def _names(k):
    return [f"s{i + 1}" for i in range(k)]


def _compare(X, method, use="pairwise.complete.obs", alternative="two.sided", continuity=False, include_only=None):
    names = _names(X.shape[1])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = cor_fast(X, use=use, method=method, alternative=alternative, continuity=continuity,
                       include_only=include_only, colnames=names, return_matrix=False)["rho"]
    pi, pj, _ = api.setup_comparisons(names, include_only, diag_good=False)
    Xc = X
    if use == "complete.obs":
        Xc = X[~np.isnan(X).any(axis=1)]
    if use in ("everything", "all.obs") and np.isnan(X).any():
        assert np.isnan(got["rho"]).all() and np.isnan(got["pvalue"]).all()
        return got
    want, warned = check_pairs(Xc, pi, pj, method, use == "pairwise.complete.obs", alternative, continuity)
    np.testing.assert_allclose(got["rho"], want[:, 0], atol=1e-12, rtol=0, equal_nan=True)
    gp, wp = np.asarray(got["pvalue"], float), want[:, 1]
    assert np.array_equal(np.isnan(gp), np.isnan(wp))
    ok = ~np.isnan(wp)
    np.testing.assert_allclose(gp[ok], wp[ok], atol=1e-10, rtol=0)
    big = ok & (wp >= 1e-290)
    np.testing.assert_allclose(gp[big], wp[big], rtol=1e-8, atol=0)
    assert np.array_equal(np.asarray(got["n_values"], float), want[:, 2])
    assert warned == any("Cannot compute exact p-value with ties" in str(w.message) for w in rec)
    return got


def _matrix(n, S, seed, na=0.0, ties=False):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, S)) + rng.normal(size=(n, 1))
    if ties:
        X[:, ::2] = np.round(X[:, ::2] * 2)
    if na:
        X[rng.random(X.shape) < na] = np.nan
    return X


@pytest.mark.parametrize("method", ["pearson", "spearman"])
@pytest.mark.parametrize("use", ["everything", "all.obs", "complete.obs", "pairwise.complete.obs"])
@pytest.mark.parametrize("alternative", ["two.sided", "less", "greater"])
def test_methods_uses_alternatives(method, use, alternative):
    _compare(_matrix(60, 9, 1, na=0.05, ties=True), method, use, alternative)
    _compare(_matrix(60, 9, 2), method, use, alternative)


@pytest.mark.parametrize("continuity", [False, True])
@pytest.mark.parametrize("n", [8, 40, 1289, 1290, 1500])
def test_spearman_tied_untied_around_1290(n, continuity):
    for ties in (False, True):
        _compare(_matrix(n, 5, n, ties=ties), "spearman", "everything", "two.sided", continuity)
        _compare(_matrix(n, 5, n + 1, na=0.1, ties=ties), "spearman", "pairwise.complete.obs", "greater", continuity)


def test_inf_and_constant_columns():
    X = _matrix(50, 6, 3)
    X[3, 1] = np.inf
    X[7, 2] = -np.inf
    X[:, 4] = 2.5
    X[:, 5] = np.where(np.arange(50) < 25, 1.0, np.nan)    # constant on its present rows
    for method in ("pearson", "spearman"):
        _compare(X, method, "everything" if method == "spearman" else "pairwise.complete.obs")
        _compare(X, method, "pairwise.complete.obs")
    Xn = X.copy()
    Xn[3, 0] = np.nan   # the Inf row of column 2 leaves pair (1, 2) in pairwise mode
    _compare(Xn, "pearson", "pairwise.complete.obs")


def test_include_only_forms():
    X = _matrix(80, 7, 4, na=0.1)
    for inc in (["s3"], ["s1", "s5"], [["s1", "s2", "s6"], ["s4", "s7", "s6"]]):
        for method in ("pearson", "spearman"):
            _compare(X, method, "pairwise.complete.obs", include_only=inc)
            _compare(X, method, "complete.obs", include_only=inc)
    import pandas as pd
    _compare(X, "pearson", "pairwise.complete.obs", include_only=pd.DataFrame({"a": ["s1", "s2"], "b": ["s3", "s4"]}))


@pytest.mark.parametrize("frac", [0.0, 0.1, 0.3, 0.6])
def test_pairwise_na_fractions(frac):
    X = _matrix(200, 12, int(frac * 10) + 5, na=frac, ties=True)
    X[:198, 11] = np.nan      # 2 rows: fewer than 3 joint rows with every column
    for method in ("pearson", "spearman"):
        got = _compare(X, method, "pairwise.complete.obs", "less")
        short = (np.asarray(got["n_values"]) < 3)
        assert short.any() and np.isnan(np.asarray(got["rho"])[short]).all()


@pytest.mark.parametrize("n,S", [(3, 2), (4, 3), (100, 65), (1000, 130), (65535, 4), (2049, 70)])
def test_shapes(n, S):
    for method in ("pearson", "spearman"):
        _compare(_matrix(n, S, n + S), method, "everything")
        _compare(_matrix(n, S, n + S + 1, na=0.2 if n > 10 else 0.0), method, "pairwise.complete.obs")


def test_wide_columns_and_many_samples():
    X = _matrix(200000, 2, 9, na=0.05)
    for method in ("pearson", "spearman"):
        _compare(X, method, "pairwise.complete.obs")
        _compare(X, method, "complete.obs")
    X = _matrix(40, 600, 10)
    for method in ("pearson", "spearman"):
        got = cor_fast(X, method=method, colnames=_names(600), return_matrix=False)["rho"]
        pi, pj, _ = api.setup_comparisons(_names(600), None, diag_good=False)
        sub = np.random.default_rng(0).choice(len(pi), 3000, replace=False)
        want, _ = check_pairs(X, pi[sub], pj[sub], method, False)
        np.testing.assert_allclose(np.asarray(got["rho"])[sub], want[:, 0], atol=1e-12)
        np.testing.assert_allclose(np.asarray(got["pvalue"])[sub], want[:, 1], atol=1e-10)


def test_readme_on_gpu():
    from oracle.rrng import RRandom
    rr = RRandom(1234)
    rr.rnorm(1000, 100, 10)
    rr.sample(100, 50)
    rr.sample(100, 50)
    x, y = rr.rnorm(1000), rr.rnorm(1000)
    r = cor_fast(np.column_stack([x, y, x]), colnames=["s1", "s2", "s3"])
    rho, p = np.asarray(r["rho"]), np.asarray(r["pvalue"])
    assert rho[0, 1] == pytest.approx(0.00720612, abs=5e-9) and p[0, 1] == pytest.approx(0.8199608, abs=5e-8)
    assert np.all(np.diag(p) == 0) and p[0, 2] == 0 and rho[0, 2] == pytest.approx(1)


def test_bad_arguments_are_refused():
    ctx = _lib.default_context()
    X = np.zeros((5, 2))
    with pytest.raises(_lib.IciktError, match="column index out of range"):
        ctx.cor_pairs(X, [0], [2])
    with pytest.raises(_lib.IciktError, match="too long|ICIKT_MAX_FEATURES_WIDE"):
        ctx.cor_pairs(np.zeros((_lib.MAX_FEATURES_WIDE + 1, 2)), [0], [1])
