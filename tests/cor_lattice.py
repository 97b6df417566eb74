"""Designed columns for the t branch of cor_fast's p-values (test infrastructure only): matrices whose pairs (0, k)
have a correlation chosen in advance, so that a test visits the (df, t) plane on purpose -- the centre on both sides
of the continued fraction's swap point, p down to 1e-289 at every df that can reach it, |rho| -> 1 at small df, both
sides of cor_lbeta's split at df/2 = 10, df = 1 and the longest column the library takes.

The targets are chosen by p, not by rho.  scipy.stats.t.isf finds the rho of a wanted p; it only chooses the inputs.
What a result is compared with is tests/t_tail_exact.py at the rho the code under test returned."""
import math
from collections import namedtuple

import numpy as np
from scipy import stats

from tests.t_tail_exact import on_tail_side, t_pvalue_exact

ABS_BAR, REL_BAR, P_FLOOR = 1e-10, 1e-8, 1e-290     # the bars of tests/test_gpu_cor_fast.py

PEARSON_N = (3, 4, 5, 12, 21, 22, 23, 42, 1291, 20002, 65535, 262144)      # df = 1, 19 | 20 | 21, the cap
P_TARGETS = (1 - 1e-9, 0.9, 0.5, 0.1, 1e-2, 1e-4, 1e-8, 1e-16, 1e-32, 1e-64, 1e-128, 1e-256, 1e-289)
P_UNDERFLOW = 1e-305
RHO_MAX = 1 - 1e-12
SPEARMAN_CASES = ((1290, False), (1291, False), (5000, False), (12, True), (400, True), (1289, True), (1290, True))
SPEARMAN_P = (0.9, 0.5, 0.1, 1e-2, 1e-4, 1e-8, 1e-16, 1e-32, 1e-64, 1e-128, 1e-256)

# rho: the designed correlation; name: what the point is there for; underflow: one of the named points whose p is
# below P_FLOOR (or 0) and which alone may escape the relative bar
Target = namedtuple("Target", "rho name underflow")


def rho_at_p(p, df):
    """The positive rho whose two-sided t p-value over df degrees of freedom is p (to scipy's accuracy)."""
    t = float(stats.t.isf(p / 2, df))
    return t / math.sqrt(df + t * t) if math.isfinite(t) else 1.0


def swap_rho(df):
    """|rho| at the swap point of the incomplete beta function: x = 1 - rho^2 = (a + 1) / (a + b + 2) for a = df/2,
    b = 1/2, which is (df + 2) / (df + 5)."""
    return math.sqrt(3.0 / (df + 5.0))


def pearson_targets(n):
    """The designed correlations at n rows, both signs of each."""
    df = n - 2
    out = []

    def both(rho, name, underflow=False):
        out.extend(Target(s * rho, name, underflow) for s in (1.0, -1.0))

    for p in P_TARGETS:
        rho = rho_at_p(p, df)
        if rho <= RHO_MAX:
            both(rho, f"p={p:.0e}" if p < 0.5 else f"p={p!r}")
    for f in (1 + 1e-9, 1 - 1e-9):
        both(swap_rho(df) * f, f"swap*{'(1+1e-9)' if f > 1 else '(1-1e-9)'}")
    # |rho| -> 1.  Besides the two powers of two, a rho whose square does not fit a double where that hurts most:
    # for 1 - |rho| = d, rounding rho^2 costs 1 - rho^2 up to min(d / 2, 2^-54 / (2 d)) relatively, largest near
    # d = 2^-27, and p = c (1 - rho^2)^(df/2) takes df/2 times that: 3.7e-9 df/2, past REL_BAR from df = 6 on
    # unless 1 - rho^2 is formed as (1 - rho)(1 + rho) or with one fma
    near_one = ((1 - 2.0 ** -20, "1-2^-20"), (1 - 1.618 * 2.0 ** -28, "1-1.618*2^-28"), (1 - 2.0 ** -40, "1-2^-40"))
    for rho, name in near_one:
        # ten decades above the floor: p moves by (1 - rho)^(df/2) with the last bits of rho this close to 1
        if 2 * stats.t.sf(math.sqrt(df) * rho / math.sqrt((1 - rho) * (1 + rho)), df) >= 1e10 * P_FLOOR:
            both(rho, name)
    rho = rho_at_p(P_UNDERFLOW, df)
    if rho <= RHO_MAX:
        both(rho, "p=1e-305", True)
    both(1.0, "identical/negated", True)
    return out


def _basis(n, seed):
    """u, v: centred, orthogonal, each of sample standard deviation 1 (Gram-Schmidt against the ones vector and each
    other, twice)."""
    rng = np.random.default_rng(seed)
    u, v = rng.normal(size=n), rng.normal(size=n)
    for _ in range(2):
        u -= u.mean()
        u /= math.sqrt(float(u @ u))
        v -= v.mean()
        v -= float(v @ u) * u
        v /= math.sqrt(float(v @ v))
    s = math.sqrt(n - 1)
    return u * s, v * s


def _padded(X, pad, rng):
    """pad more rows in which column 0 is NaN and the others hold finite junk: the joint rows of (0, k) stay the first
    n, but their count and sums come from the pairwise kernels."""
    if not pad:
        return X
    junk = 1.0 + 3.0 * rng.normal(size=(pad, X.shape[1]))
    junk[:, 0] = np.nan
    return np.vstack([X, junk])


def _pairs(K):
    return np.zeros(K, dtype=np.int32), np.arange(1, K + 1, dtype=np.int32)


def pearson_lattice(n, targets, pad=0):
    """(X, pi, pj): column 0 = u, column k = r_k u + sqrt(1 - r_k^2) v for targets[k - 1].rho = r_k, pairs (0, k)."""
    u, v = _basis(n, 1000 + n)
    X = np.empty((n, len(targets) + 1))
    X[:, 0] = u
    for k, tg in enumerate(targets, 1):
        r = tg.rho
        X[:, k] = r * u + math.sqrt((1 - r) * (1 + r)) * v
    pi, pj = _pairs(len(targets))
    return _padded(X, pad, np.random.default_rng(n)), pi, pj


def spearman_lattice(n, tied, pad=0):
    """(X, pi, pj): column 0 = x, column k a strictly monotone map of r_k x + sqrt(1 - r_k^2) noise_k, with r_k of both
    signs at the rho of SPEARMAN_P (|r_k| <= 0.9), so that Spearman's rho of the pairs (0, k) spreads over both tails
    and the centre.  tied: every column rounded to max(n // 4, 3) levels of its ranks."""
    df = n - 2
    rs = sorted({s * r for p in SPEARMAN_P for s in (1, -1) for r in [rho_at_p(p, df)] if r <= 0.9})
    rng = np.random.default_rng(2000 + n + tied)
    x = rng.normal(size=n)
    X = np.empty((n, len(rs) + 1))
    X[:, 0] = x
    for k, r in enumerate(rs, 1):
        z = r * x + math.sqrt(1 - r * r) * rng.normal(size=n)
        X[:, k] = z * z * z + z
    if tied:
        levels = max(n // 4, 3)
        ranks = np.argsort(np.argsort(X, axis=0), axis=0)
        X = np.floor(ranks * (levels / n))
    pi, pj = _pairs(len(rs))
    return _padded(X, pad, np.random.default_rng(n)), pi, pj


def assert_spearman_spread(rho, n):
    """The rank columns reach both tails and the centre: a two-sided p <= 1e-100 on either side of 0 (1e-3 where n is
    too short for that) and one >= 0.3."""
    p = np.array([float(t_pvalue_exact(float(r), n - 2)) for r in rho])
    far = 1e-100 if n >= 400 else 1e-3
    assert p[rho > 0].min() <= far and p[rho < 0].min() <= far and p.max() >= 0.3, (n, p.min(), p.max())


def compare_with_exact(rho, pv, df, alternative, designed, label=""):
    """Hold p-values to tests/t_tail_exact.py at the rho they were computed from: |d| <= ABS_BAR everywhere, and
    relative REL_BAR wherever the p-value is a tail (not a complement) and the reference is >= P_FLOOR.  designed[k]:
    point k is meant to be checked relatively (when on its tail side); exactly those points must be, so a lattice
    that slid below the floor fails here instead of passing unchecked.  Prints the worst figures before it asserts
    and returns (number checked relatively, the worst relative error, the index where it occurred)."""
    rho, pv = np.asarray(rho, dtype=np.float64), np.asarray(pv, dtype=np.float64)
    assert not np.isnan(rho).any() and not np.isnan(pv).any(), label
    worst, where, worst_abs, where_abs, checked = 0.0, -1, 0.0, -1, []
    for k in range(len(rho)):
        ref = t_pvalue_exact(float(rho[k]), df, alternative)
        d = abs(float(pv[k] - ref))
        if d > worst_abs:
            worst_abs, where_abs = d, k
        if on_tail_side(float(rho[k]), alternative) and ref >= P_FLOOR:
            rel = abs(float(pv[k] / ref - 1))
            checked.append(k)
            if rel > worst:
                worst, where = rel, k
    at = f"rho = {rho[where]!r}, p = {pv[where]:.3g}" if where >= 0 else "-"
    print(f"{label} df = {df} {alternative}: {len(checked)} relative, worst {worst:.3g} at {at}; "
          f"worst |d| {worst_abs:.3g}")
    assert worst_abs <= ABS_BAR, f"{label} df = {df}: |d| = {worst_abs:.3g} at rho = {rho[where_abs]!r}"
    want = [k for k in range(len(rho)) if designed[k] and on_tail_side(float(rho[k]), alternative)]
    assert checked == want, f"{label} df = {df}: checked relatively {checked}, designed {want}"
    assert worst <= REL_BAR, f"{label} df = {df}: relative {worst:.3g} at {at}"
    return len(checked), worst, where
