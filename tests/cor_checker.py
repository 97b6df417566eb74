"""CPU checker of cor_fast (test infrastructure only): estimates from scipy's pearsonr / spearmanr, p-values from the
regularized incomplete beta (scipy's betainc, mpmath's at 50 digits in the spot checks), Spearman's exact p-value by
enumerating permutations.  Two pieces have no independent implementation here and no R to compare with: the AS 89
Edgeworth series (10 <= n < 1290, no ties) and Spearman's continuity correction -- for those the checker takes the
front end's own restatement (icikendalltau_amd.api), as DESIGN.md section 9 says."""
import itertools
import math

import numpy as np
from scipy import special, stats

from icikendalltau_amd import api

_UPPER = {}


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
    tail = 0.0 if math.isinf(t) else 0.5 * float(special.betainc(df / 2, 0.5, df / (df + t * t)))
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
            return api._prho(round(q) + 2 * lower, n, lower)          # Edgeworth: unpinned restatement
        r = 1 - q / den
        if continuity and r != 0:
            r -= math.copysign(1.0, r) / den                          # unpinned restatement
        with np.errstate(divide="ignore"):
            t = float(r / np.sqrt(np.float64((1 - r * r) / (n - 2)))) if n > 2 else math.nan
        return t_pvalue(t, n - 2, "less" if not lower else "greater")

    if alternative == "two.sided":
        return min(2 * ps(not (q > den)), 1.0)
    return ps(alternative == "greater")


def check_pairs(X, pi, pj, method, pairwise, alternative="two.sided", continuity=False):
    """(rho, p, n_values) per pair and whether any pair warned about ties."""
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
            # two-pass centred sums and one division, as R's cor: identical vectors give rho = 1 exactly
            xc, yc = x - x.mean(), y - y.mean()
            rho = float(np.clip((xc * yc).sum() / math.sqrt((xc * xc).sum() * (yc * yc).sum()), -1, 1))
            assert abs(rho - stats.pearsonr(x, y).statistic) < 1e-13
            out[p, 0] = rho
            with np.errstate(divide="ignore"):
                t = float(np.sqrt(np.float64(n - 2)) * rho / np.sqrt(np.float64(1 - rho * rho)))
            out[p, 1] = t_pvalue(t, n - 2, alternative)
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
