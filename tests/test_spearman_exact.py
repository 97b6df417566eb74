"""``api._prho`` (AS 89, the restatement the device epilogue mirrors) against the exact permutation distribution of
Spearman's S (tests/spearman_exact.py), exhaustively: every attainable ``is`` and both tails at n = 10 .. 16, and the
tabulated branch at n <= 9.

Two caps hold the Edgeworth branch.  (a) worst |p - exact| <= 1.25 x ``AS89_ERROR[n]``, the series' own departure
from the truth: the margin covers libm differences and the single-point maximum, and stays below the smallest effect
of a 5 % error in c1 or c4 (1.33 x).  (b) at least 20 times better than the plain normal tail at the same x, computed
here from scipy and the exact distribution alone (a correct series is 22 x better at n = 10, 211 x at n = 16).
The mutation tests show that (a) has teeth: a local copy of the series with c1 off by 5 % or with ``is`` in place of
``is - 1`` breaks it.  The b^2 and b^3 coefficients (c3, c6, c8, c12) stay invisible at these caps."""
import math

import numpy as np
import pytest
from scipy import stats

from icikendalltau_amd import api
from tests import spearman_exact as SE
from tests.cor_checker import exact_upper

AS89 = (0.2274, 0.2531, 0.1745, 0.0758, 0.1033, 0.3932, 0.0879, 0.0151, 0.0072, 0.0831, 0.0131, 4.6e-4)


def _x(is_, n, shift=1.0):
    return (6.0 * (is_ - shift) / (n * (n * n - 1.0)) - 1.0) * math.sqrt(n - 1.0)


def _series(is_, n, lower, c=AS89, shift=1.0):
    """The Edgeworth series as DESIGN.md section 9 quotes it, with its coefficients and lattice shift open to
    mutation; the normal tails come from scipy."""
    b = 1.0 / n
    x = _x(is_, n, shift)
    y = x * x
    u = x * b * (c[0] + b * (c[1] + c[2] * b) + y * (-c[3] + b * (c[4] + c[5] * b) - y * b * (
        c[6] + c[7] * b - y * (c[8] - c[9] * b + y * b * (c[10] - c[11] * y)))))
    e = u * math.exp(-y / 2)
    return min(1.0, max(0.0, stats.norm.cdf(x) - e if lower else stats.norm.sf(x) + e))


def _worst(fn, n):
    """max |fn(is, n, lower) - exact| over every even is = 2 .. S_max and both tails: P[S >= is], P[S < is]."""
    up = SE.upper(n)
    worst = 0.0
    for k in range(1, len(up)):
        worst = max(worst, abs(fn(2 * k, n, False) - up[k]), abs(fn(2 * k, n, True) - (1.0 - up[k])))
    return worst


@pytest.mark.parametrize("n", range(2, 9))
def test_dp_counts_equal_enumeration(n):
    cnt = SE.s_counts(n)
    assert len(cnt) == (n ** 3 - n) // 6 + 1 and cnt.dtype == np.int64
    for k in range(len(cnt) + 1):
        ge, fact = exact_upper(n, 2 * k)
        assert fact == math.factorial(n) and ge == int(cnt[k:].sum()), (n, k)


def test_tail_helpers():
    n = 6
    cnt, top, fact = SE.s_counts(n), SE.s_max(n), math.factorial(n)
    assert top == 70 and cnt[0] == 1 and cnt[-1] == 1 and cnt[1] == n - 1
    assert np.array_equal(cnt, cnt[::-1])                               # S and S_max - S are equally distributed
    assert SE.p_ge(n, 0) == 1.0 and SE.p_le(n, top) == 1.0 and SE.p_ge(n, top) == 1 / fact == SE.p_le(n, 0)
    for s in range(0, top + 1, 2):
        assert SE.p_le(n, s) + SE.p_ge(n, s + 2) == pytest.approx(1.0, abs=1e-15)
        assert SE.pvalue(n, s, "greater") == SE.p_le(n, s) and SE.pvalue(n, s, "less") == SE.p_ge(n, s)
        assert SE.pvalue(n, s, "two.sided") == min(1.0, 2 * min(SE.p_le(n, s), SE.p_ge(n, s)))
    assert SE.pvalue(n, 34, "two.sided") == min(1.0, 2 * SE.p_le(n, 34))  # 34 < the mean 35: the lower tail
    assert SE.pvalue(n, 36, "two.sided") == min(1.0, 2 * SE.p_ge(n, 36))


@pytest.mark.parametrize("n", [10, 13, 16])
def test_ladder_covers_tails_and_centre(n):
    perms = SE.ladder(n, np.random.default_rng(6))          # asserts its own conditions
    assert all(sorted(p.tolist()) == list(range(n)) for p in perms) and len(perms) == 42 + 2 * (n // 2)
    s = np.array([SE.s_of(p) for p in perms])
    mean = SE.s_max(n) / 2
    sd = mean / math.sqrt(n - 1)                            # var(rho) = 1 / (n - 1), S = mean (1 - rho)
    assert (np.abs(s - mean) < sd).sum() >= 10              # the centre: 27 of the 40 random ones are expected there


@pytest.mark.parametrize("n", range(2, 10))
def test_table_branch_is_exact(n):
    up, cnt, fact = SE.upper(n), SE.s_counts(n), math.factorial(n)
    for k in range(1, len(up)):
        assert api._prho(2 * k, n, False) == pytest.approx(up[k], rel=1e-15, abs=0)
        assert api._prho(2 * k, n, True) == pytest.approx(int(cnt[:k].sum()) / fact, rel=1e-15, abs=0)
        assert api._prho(2 * k - 1, n, False) == pytest.approx(up[k], rel=1e-15, abs=0)   # odd is: the next even S


@pytest.mark.parametrize("n", range(10, 17))
def test_edgeworth_branch_within_as89s_own_error(n):
    up = SE.upper(n)
    got = _worst(api._prho, n)
    normal = max(abs(stats.norm.sf(_x(2 * k, n)) - up[k]) for k in range(1, len(up)))
    print(f"n = {n}: worst |_prho - exact| = {got:.4g} ({got / SE.AS89_ERROR[n]:.3f} x table), "
          f"normal tail {normal:.4g} ({normal / got:.1f} x)")
    assert got <= 1.25 * SE.AS89_ERROR[n]                   # (a)
    assert got <= normal / 20                               # (b)


def test_local_series_is_the_restatement():
    """The copy the mutation tests perturb is the series under test, to libm differences."""
    for n in (10, 16, 400, 1289):
        for is_ in np.linspace(2, SE.s_max(n) if n <= 16 else (n ** 3 - n) // 3, 60).astype(np.int64):
            for lower in (False, True):
                assert _series(int(is_), n, lower) == pytest.approx(api._prho(int(is_), n, lower), abs=1e-14)


def test_cap_catches_five_percent_on_c1():
    c = list(AS89)
    c[0] *= 1.05
    assert _worst(_series, 16) <= 1.25 * SE.AS89_ERROR[16]
    assert _worst(lambda i, n, lo: _series(i, n, lo, tuple(c)), 16) > 1.25 * SE.AS89_ERROR[16]


def test_cap_catches_a_lattice_step():
    assert _worst(_series, 10) <= 1.25 * SE.AS89_ERROR[10]
    assert _worst(lambda i, n, lo: _series(i, n, lo, shift=0.0), 10) > 1.25 * SE.AS89_ERROR[10]


@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("n", [5, 9, 10, 11, 13, 16])
def test_numpy_path_on_the_ladder(n, pad):
    """The front end's numpy path (engines without cor_pairs) from data to p, on the columns the device test uses."""
    worst = SE.ladder_errors(api._cor_pairs_numpy, n, pad)
    SE.assert_ladder_within_as89(worst, n, "numpy")
