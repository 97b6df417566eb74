"""cor_fast's Pearson arithmetic on the MI355X against exact arithmetic (tests/cor_checker.py, exact_pearson) on data
where double-precision formulas go wrong: offsets far beyond the spread, columns near 1e+-300, a pair's rows far from
its columns' means, a pair whose only spread is two adjacent doubles.  Every Pearson branch of icikt_cor_pairs_f64 is
reached on purpose: the tile kernel (the full combn list, no NA), k_cor_dots<false> (any other list, no NA),
k_cor_dots<true> (pairwise), and complete.obs (the front end drops rows, then a dense branch).  rho |d| <= 1e-12,
p as tests/test_gpu_cor_fast.py pins it at the exact rho, n_values and reason codes exact.  At the 262 144-row limit
y = x and y = -x give rho = +-1 exactly, for Pearson and Spearman, dense and pairwise."""
import functools

import numpy as np
import pytest

from icikendalltau_amd import _lib, api, cor_fast
from tests.cor_checker import assert_matches_exact, check_pairs, ill_dense, ill_pairwise

pytestmark = pytest.mark.gpu

NS = [3, 64, 65, 2000, 65536, 200000]
ALTS = ("two.sided", "less", "greater")


def _alt(n):
    return ALTS[NS.index(n) % 3]


def _full_list(S):
    """combn(S, 2) then the S self pairs: the list the host hands to the tile kernel."""
    names = [f"s{i}" for i in range(S)]
    pi, pj, _ = api.setup_comparisons(names, None, diag_good=False)
    return pi, pj


def _reasons(want):
    r = np.full(len(want), _lib.COR_OK, dtype=np.int32)
    r[np.isnan(want[:, 0])] = _lib.COR_NA
    r[want[:, 2] < 3] = _lib.COR_SHORT
    return r


@functools.lru_cache(maxsize=1)
def _dense_case(n):
    X = ill_dense(n, n)
    pi, pj = _full_list(X.shape[1])
    want, _ = check_pairs(X, pi, pj, "pearson", False, _alt(n), exact=True)
    return X, pi, pj, want


def _check(ctx, X, pi, pj, want, pairwise, alternative, label):
    out, rsn = ctx.cor_pairs(X, pi, pj, "pearson", pairwise, alternative)
    assert_matches_exact(out[:, 0], out[:, 1], out[:, 2], want, alternative, label)
    assert np.array_equal(rsn, _reasons(want)), label


@pytest.mark.parametrize("n", NS)
def test_dense_branches(hip_ctx, n):
    X, pi, pj, want = _dense_case(n)
    alt = _alt(n)
    _check(hip_ctx, X, pi, pj, want, False, alt, f"tile n={n}")
    rev = slice(None, None, -1)   # the same pairs in another order: not the full list, so one wave per pair
    _check(hip_ctx, X, pi[rev], pj[rev], want[rev], False, alt, f"dots n={n}")
    _check(hip_ctx, X, pi, pj, want, True, alt, f"pairwise without NA n={n}")
    S = X.shape[1]
    assert (want[len(pi) - S:, 0] == 1).all()


@pytest.mark.parametrize("n", NS)
def test_complete_obs(n):
    X, pi, pj, want = _dense_case(n)
    S = X.shape[1]
    # rows with an NA between the data rows: complete.obs drops them and computes X's pairs on a dense branch
    Xn = np.full((n + S, S), np.nan)
    keep = np.ones(n + S, dtype=bool)
    at = np.linspace(0, n + S - 1, S).astype(int)
    keep[at] = False
    Xn[keep] = X
    Xn[at] = 1.0
    Xn[at, np.arange(S)] = np.nan
    names = [f"s{i}" for i in range(S)]
    got = cor_fast(Xn, use="complete.obs", alternative=_alt(n), colnames=names, return_matrix=False)["rho"]
    assert_matches_exact(got["rho"], got["pvalue"], got["n_values"], want, _alt(n), f"complete.obs n={n}")
    inc = [["s1", "s7", "s3"], ["s2", "s8", "s10"]]
    got = cor_fast(Xn, use="complete.obs", alternative=_alt(n), include_only=inc, colnames=names,
                   return_matrix=False)["rho"]
    ipi, ipj, _ = api.setup_comparisons(names, inc, diag_good=False)
    sel = [int(np.flatnonzero((pi == a) & (pj == b))[0]) for a, b in zip(ipi, ipj)]
    assert_matches_exact(got["rho"], got["pvalue"], got["n_values"], want[sel], _alt(n), f"include_only n={n}")


@pytest.mark.parametrize("n", NS)
def test_pairwise(hip_ctx, n):
    X = ill_pairwise(n, n + 1)
    pi, pj = _full_list(X.shape[1])
    alt = _alt(n)
    want, _ = check_pairs(X, pi, pj, "pearson", True, alt, exact=True)
    _check(hip_ctx, X, pi, pj, want, True, alt, f"pairwise n={n}")
    if n >= 64:   # the front end takes the same path
        names = [f"s{i}" for i in range(X.shape[1])]
        got = cor_fast(X, use="pairwise.complete.obs", alternative=alt, colnames=names, return_matrix=False)["rho"]
        assert_matches_exact(got["rho"], got["pvalue"], got["n_values"], want, alt, f"front end n={n}")


def test_pairwise_adjacent_doubles_are_not_constant(hip_ctx):
    """The subset's only spread is one ulp while its column holds an outlier: a finite rho, not a zero variance."""
    n = 2000
    X = ill_pairwise(n, 5)
    out, rsn = hip_ctx.cor_pairs(X, [5], [6], "pearson", True)
    want, _ = check_pairs(X, [5], [6], "pearson", True, exact=True)
    assert rsn[0] == _lib.COR_OK and np.isfinite(want[0, 0])
    assert_matches_exact(out[:, 0], out[:, 1], out[:, 2], want, label="adjacent doubles")


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_length_limit_exact_signs(hip_ctx, method):
    """n = 262 144: y = x and y = -x give rho = +-1 exactly.  The columns' Pearson sums (heavily tied {0, 1, 2, 3},
    and a permutation of 0 .. n - 1, whose sums of squares come within 2^53 in units of 1/4) and every Spearman sum
    are exact in f64 at this length, on the dense paths and the pairwise ones; the NA columns' pairs are exact by
    symmetry."""
    n = _lib.MAX_FEATURES_WIDE
    assert n == 262144
    rng = np.random.default_rng(3)
    r = np.arange(n)
    t = (r % 4).astype(np.float64)
    u = rng.permutation(n).astype(np.float64)
    w = rng.normal(size=n) + 1e6
    w[rng.random(n) < 0.1] = np.nan
    X = np.column_stack([t, t, -t, u, u, -u, w, w, -w])
    sign = np.array([1.0, -1.0, -1.0])
    # dense: the full list of the six NA-free columns (tile) and the identity pairs alone (one wave per pair)
    pi, pj = _full_list(6)
    X6 = X[:, :6]
    out, rsn = hip_ctx.cor_pairs(X6, pi, pj, method, False)
    want, _ = check_pairs(X6, pi, pj, method, False, exact=method == "pearson")
    assert (rsn == _lib.COR_OK).all() and (out[:, 2] == n).all()
    if method == "pearson":
        assert_matches_exact(out[:, 0], out[:, 1], out[:, 2], want, label="limit tile")
    else:
        np.testing.assert_allclose(out[:, 0], want[:, 0], atol=1e-12, rtol=0)
    qi, qj = np.array([0, 0, 1, 3, 3, 4]), np.array([1, 2, 2, 4, 5, 5])
    for a, b, s in zip(qi, qj, np.tile(sign, 2)):
        k = int(np.flatnonzero((pi == a) & (pj == b))[0])
        assert out[k, 0] == s and out[k, 1] == 0.0, ("tile", a, b, out[k])
    out, rsn = hip_ctx.cor_pairs(X6, qi, qj, method, False)
    assert (out[:, 0] == np.tile(sign, 2)).all() and (out[:, 1] == 0).all() and (rsn == _lib.COR_OK).all(), out
    # pairwise: the same pairs and the NA columns' (6, 7, 8)
    qi, qj = np.r_[qi, 6, 6, 7], np.r_[qj, 7, 8, 8]
    out, rsn = hip_ctx.cor_pairs(X, qi, qj, method, True)
    assert (out[:, 0] == np.tile(sign, 3)).all() and (out[:, 1] == 0).all() and (rsn == _lib.COR_OK).all(), out
    nw = int((~np.isnan(w)).sum())
    assert (out[:, 2] == np.r_[np.full(6, n), np.full(3, nw)]).all()
