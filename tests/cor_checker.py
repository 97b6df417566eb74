"""CPU checker of cor_fast (test infrastructure only): estimates from scipy's pearsonr / spearmanr, p-values from the
regularized incomplete beta (scipy's betainc, mpmath's at 50 digits in the spot checks), Spearman's exact p-value by
enumerating permutations.  Two pieces have no independent implementation in this module and no R to compare with:
the AS 89 Edgeworth series (10 <= n < 1290, no ties) and Spearman's continuity correction -- for those the checker
takes the front end's own restatement (icikendalltau_amd.api).  The series itself is pinned elsewhere, as DESIGN.md
section 9 says: tests/spearman_exact.py holds ``api._prho`` and the device to the exact permutation distribution at
n = 10 .. 16 within AS 89's own error, and to the t tail at n = 1289; the continuity correction stays unpinned.
The t tail itself (every Pearson p-value, Spearman's with ties or at n >= 1290) is held here to scipy's betainc only at
the rho the data happens to have; tests/t_tail_exact.py holds ``api.cor_test_pvalue`` and the device to a series at
400 digits on the designed (n, rho) lattice of tests/cor_lattice.py.

For ill-conditioned data (large offsets, extreme scales, a pair's rows far from its column's mean) scipy is no
reference: ``exact_pearson`` is, Pearson's rho of the given doubles in exact integer arithmetic, rounded once."""
import itertools
import math

import mpmath
import numpy as np
from scipy import special, stats

from icikendalltau_amd import api

_UPPER = {}


def _dyadic(v):
    """Finite doubles v as Python ints a_k with v_k = a_k * 2**e, one e for the whole vector."""
    f, ex = np.frexp(np.asarray(v, dtype=np.float64))     # v = f * 2**ex, 0.5 <= |f| < 1
    mant = (f * 2.0 ** 53).astype(np.int64)                # exact: f has at most 53 significant bits
    ex = ex.astype(np.int64) - 53
    nz = mant != 0
    e0 = int(ex[nz].min()) if nz.any() else 0
    sh = np.where(nz, ex - e0, 0)
    return [m << s for m, s in zip(mant.tolist(), sh.tolist())]


def exact_pearson(x, y):
    """Pearson's rho of two equal-length vectors of finite doubles, from exact sums: every double is a dyadic
    rational, so m Sxx = m sum a^2 - (sum a)^2 (and Syy, Sxy alike) are integers on a common scale.  rho =
    m Sxy / sqrt(m Sxx m Syy) at 200 bits (the scales cancel), rounded once to a double.  NaN when a side has no
    variance or fewer than 2 rows."""
    a, b = _dyadic(x), _dyadic(y)
    m = len(a)
    if m < 2 or m != len(b):
        return math.nan
    sa, sb = sum(a), sum(b)
    A = m * sum(v * v for v in a) - sa * sa
    B = m * sum(v * v for v in b) - sb * sb
    C = m * sum(u * v for u, v in zip(a, b)) - sa * sb
    if A == 0 or B == 0:
        return math.nan
    with mpmath.workprec(200):
        return float(mpmath.mpf(C) / mpmath.sqrt(mpmath.mpf(A) * mpmath.mpf(B)))


def exact_upper(n, is_):
    """#permutations of n rows with S = sum (i - perm(i))^2 >= is_, and n!."""
    if n not in _UPPER:
        base = np.arange(n)
        _UPPER[n] = np.array(sorted(int(((base - np.asarray(p)) ** 2).sum()) for p in itertools.permutations(range(n))))
    s = _UPPER[n]
    return int((s >= is_).sum()), len(s)


def t_pvalue(t, df, alternative):
    if math.isnan(t) or not df > 0:
        return math.nan
    if math.isinf(t):
        tail = 0.0
    elif t * t < df:   # x = df / (df + t^2) near 1: from 1 - x = t^2 / (df + t^2), which rounding has not flattened
        tail = 0.5 * float(special.betaincc(0.5, df / 2, t * t / (df + t * t)))
    else:
        tail = 0.5 * float(special.betainc(df / 2, 0.5, df / (df + t * t)))
    if alternative == "two.sided":
        return 2 * tail
    lower = alternative == "less"
    return tail if lower == (t < 0) else 1 - tail


def spearman_pvalue(rho, n, alternative, continuity, ties):
    den = (n ** 3 - n) / 6
    q = den * (1 - rho)

    def ps(lower):
        if n < 1290 and not ties:
            if n <= 9:
                is_ = round(q) + 2 * lower
                if is_ <= 0:
                    return 0.0 if lower else 1.0
                up, fact = exact_upper(n, is_)
                return (fact - up) / fact if lower else up / fact
            return api._prho(round(q) + 2 * lower, n, lower)          # Edgeworth: pinned in tests/spearman_exact.py
        r = 1 - q / den
        if continuity and r != 0:
            r -= math.copysign(1.0, r) / den                          # unpinned restatement
        with np.errstate(divide="ignore"):
            t = float(r / np.sqrt(np.float64((1 - r * r) / (n - 2)))) if n > 2 else math.nan
        return t_pvalue(t, n - 2, "less" if not lower else "greater")

    if alternative == "two.sided":
        return min(2 * ps(not (q > den)), 1.0)
    return ps(alternative == "greater")


def pearson_pvalue(rho, n, alternative):
    """cor.test's Pearson p-value at rho over n rows (t = sqrt(n - 2) rho / sqrt(1 - rho^2), df = n - 2)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = float(np.sqrt(np.float64(n - 2)) * rho / np.sqrt(np.float64((1 - rho) * (1 + rho))))
    return t_pvalue(t, n - 2, alternative)


def check_pairs(X, pi, pj, method, pairwise, alternative="two.sided", continuity=False, exact=False):
    """(rho, p, n_values) per pair and whether any pair warned about ties.  exact (Pearson): rho from exact_pearson
    and p at that rho, with no scipy cross-check -- for data where double-precision formulas are no reference."""
    P = len(pi)
    out = np.full((P, 3), np.nan)
    warned = False
    for p in range(P):
        x, y = X[:, pi[p]], X[:, pj[p]]
        ok = ~np.isnan(x) & ~np.isnan(y)
        x, y = x[ok], y[ok]
        n = len(x)
        out[p, 2] = n
        if n < (3 if (pairwise or method == "pearson") else 2):
            continue
        if np.all(x == x[0]) or np.all(y == y[0]):
            continue
        if method == "pearson":
            if not (np.isfinite(x).all() and np.isfinite(y).all()):
                continue
            if exact:
                out[p, 0] = exact_pearson(x, y)
                out[p, 1] = pearson_pvalue(out[p, 0], n, alternative)
                continue
            # two-pass centred sums and one division, as R's cor: identical vectors give rho = 1 exactly
            xc, yc = x - x.mean(), y - y.mean()
            rho = float(np.clip((xc * yc).sum() / math.sqrt((xc * xc).sum() * (yc * yc).sum()), -1, 1))
            assert abs(rho - stats.pearsonr(x, y).statistic) < 1e-13
            out[p, 0] = rho
            out[p, 1] = pearson_pvalue(rho, n, alternative)
        else:
            # doubled average ranks are integers: exact sums, then the one rounding of sxy / sqrt(sxx syy) (R's
            # long-double cor of two rank vectors gives rho = 1 exactly for identical ones as well)
            rx = (2 * stats.rankdata(x)).astype(np.int64) - (n + 1)
            ry = (2 * stats.rankdata(y)).astype(np.int64) - (n + 1)
            sxy, sxx, syy = (int(v) for v in ((rx * ry).sum(), (rx * rx).sum(), (ry * ry).sum()))
            rho = float(np.clip(sxy / math.sqrt(float(sxx) * float(syy)), -1, 1))
            assert abs(rho - stats.spearmanr(x, y).statistic) < 1e-13
            ties = len(np.unique(x)) < n or len(np.unique(y)) < n
            warned |= ties and n < 1290
            out[p, 0] = rho
            out[p, 1] = spearman_pvalue(rho, n, alternative, continuity, ties)
    return out, warned


# ---- ill-conditioned Pearson data (numerics) ----------------------------------------------------

def _factor_columns(rng, n, S, rho):
    """S columns of n rows, every pair with true correlation rho (one shared factor)."""
    return math.sqrt(rho) * rng.normal(size=(n, 1)) + math.sqrt(1 - rho) * rng.normal(size=(n, S))


def true_rho(n):
    """A moderate true rho at which cor.test's p-value stays meaningful (t of a few units up to ~20) at n rows."""
    return min(0.45, 5 / math.sqrt(n))


def ill_dense(n, seed):
    """Columns without NA for the dense paths: offsets of both signs far beyond the spread (the rounding of the column
    mean matters), and whole columns near 1e300 and 1e-300 (squares overflow / underflow); (7, 8) mixes the two."""
    rng = np.random.default_rng(seed)
    B = _factor_columns(rng, n, 11, true_rho(n))
    X = np.empty_like(B)
    X[:, 0] = B[:, 0]
    X[:, 1], X[:, 2] = 1e12 + B[:, 1], -1e12 + B[:, 2]
    X[:, 3], X[:, 4] = 1e6 + 1e-6 * B[:, 3], -1e6 + 1e-6 * B[:, 4]
    X[:, 5], X[:, 6] = 1e10 + 1e-3 * B[:, 5], -1e10 + 1e-3 * B[:, 6]
    X[:, 7] = B[:, 7] * (1e300 / np.abs(B[:, 7]).max())
    X[:, 8] = B[:, 8] * 1e-300
    X[:, 9] = -B[:, 9] * (1e300 / np.abs(B[:, 9]).max())
    X[:, 10] = 3e-300 + B[:, 10] * 1e-301
    return X


def ill_pairwise(n, seed):
    """Columns with NA for the pairwise path, where a pair's rows sit far from its columns' means:
    (1, 0) one value 1e9 in a row where column 0 is NA; (2, 3) the first half of column 2 +1e6 where column 3 is NA
    (a censored block); (4, 0) one value 1e250 in a row column 0 lacks; (5, 6) column 5 takes two adjacent doubles on
    the rows column 6 has and 1e6 on the others; 7 .. 10 offsets and 1e+-300 scales with 10 % NA at random."""
    rng = np.random.default_rng(seed)
    B = _factor_columns(rng, n, 11, true_rho(n))
    r = np.arange(n)
    X = B.copy()
    X[r % 10 == 0, 0] = np.nan
    X[0, 1] = 1e9                                   # row 0: NA in column 0
    X[r < n // 2, 2] += 1e6
    X[r < n // 2, 3] = np.nan
    X[0, 4] = 1e250
    out6 = r % 7 == 3
    X[:, 5] = np.where(B[:, 5] > 0, np.nextafter(1.0, 2.0), 1.0)
    X[out6, 5] = 1e6
    X[out6, 6] = np.nan
    X[:, 7], X[:, 8] = 1e12 + B[:, 7], -1e12 + B[:, 8]
    X[:, 9] = B[:, 9] * (1e300 / np.abs(B[:, 9]).max())
    X[:, 10] = B[:, 10] * 1e-300
    X[:, 7:][rng.random((n, 4)) < 0.1] = np.nan
    return X


def assert_matches_exact(rho, pv, n_values, want, alternative="two.sided", label=""):
    """Device (or numpy path) results against check_pairs(..., exact=True): rho |d| <= 1e-12, n_values exact, p |d| <=
    1e-10 and <= 1e-8 relative where p >= 1e-290, p taken at the exact rho.  Where p is so ill-conditioned in rho that
    one ulp of rho moves it by more than 1e-9 relative (rho within ~1e-12 of +-1 at a few rows), it is taken at the
    tested rho instead: rho itself is pinned above, and no double estimate can do better."""
    rho, pv, n_values = (np.asarray(v, dtype=np.float64) for v in (rho, pv, n_values))
    d = np.abs(rho - want[:, 0])
    bad = ~((d <= 1e-12) | (np.isnan(rho) & np.isnan(want[:, 0])))
    assert not bad.any(), f"{label} rho: pairs {np.flatnonzero(bad)[:8].tolist()}, max |d rho| = {np.nanmax(d[bad])!r}"
    assert np.array_equal(n_values, want[:, 2]), label
    wp = want[:, 1].copy()
    for k in np.flatnonzero(~np.isnan(wp) & (wp > 0)):
        n, r = int(want[k, 2]), want[k, 0]
        side = [pearson_pvalue(np.nextafter(r, t), n, alternative) for t in (-2.0, 2.0)]
        if max(abs(s - wp[k]) for s in side) > 1e-9 * wp[k]:
            wp[k] = pearson_pvalue(float(rho[k]), n, alternative)
    assert np.array_equal(np.isnan(pv), np.isnan(wp)), label
    ok = ~np.isnan(wp)
    np.testing.assert_allclose(pv[ok], wp[ok], atol=1e-10, rtol=0, err_msg=label)
    big = ok & (wp >= 1e-290)
    np.testing.assert_allclose(pv[big], wp[big], rtol=1e-8, atol=0, err_msg=label)
