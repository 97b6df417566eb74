"""The exact null distribution of Spearman's S = sum (rank x - rank y)^2 over n untied rows (test infrastructure
only, no GPU), up to n = 16: what AS 89's Edgeworth series (``api._prho``, ``prho`` of csrc/icikt_cor.hip)
approximates for n >= 10, built without any of that series' notes.

S = 2 (sum i^2 - T) with T = sum i * perm(i), so the distribution of T is all that is needed.  A subset DP gives it:
after the first ``pos`` rows are placed, the state is the set of values used so far, and per set one polynomial in T
(int64 counts, n! = 2.1e13 at n = 16).  Layer ``pos`` holds C(n, pos) sets; the widest layer at n = 16 is 12 870
vectors of 1 497 counts, about 150 MB, and the whole table takes a few seconds.

``AS89_ERROR[n]`` is the worst |Edgeworth - exact| over every attainable S and either tail, measured once with a
transcription of the published series against this distribution: AS 89's own departure from the truth, not a property
of the code under test.  DESIGN.md section 9 says what a cap near it catches and what it does not."""
import math

import numpy as np

N_MAX = 16            # C(16, 8) vectors of 1 497 int64 ~ 150 MB; every further row doubles it

AS89_ERROR = {10: 5.603e-4, 11: 3.252e-4, 12: 1.927e-4, 13: 1.169e-4, 14: 7.238e-5, 15: 4.803e-5, 16: 3.423e-5}

_COUNTS = {}


def s_max(n):
    return (n ** 3 - n) // 3


def s_counts(n):
    """cnt[k] = permutations of n rows with S = 2 k, k = 0 .. (n^3 - n) / 6 (int64; the sum is n!)."""
    if n in _COUNTS:
        return _COUNTS[n]
    assert 1 <= n <= N_MAX
    max_t = n * (n + 1) * (2 * n + 1) // 6                  # T of the identity
    first = np.zeros(max_t + 1, dtype=np.int64)
    first[0] = 1
    layer = {0: first}
    for pos in range(1, n + 1):                             # row pos takes one of the values not yet used
        nxt = {}
        for mask, vec in layer.items():
            for v in range(n):
                if mask >> v & 1:
                    continue
                shift = pos * (v + 1)
                tgt = nxt.get(mask | 1 << v)
                if tgt is None:
                    tgt = nxt[mask | 1 << v] = np.zeros(max_t + 1, dtype=np.int64)
                tgt[shift:] += vec[:max_t + 1 - shift]
        layer = nxt
    by_t = layer[(1 << n) - 1]
    cnt = np.zeros(s_max(n) // 2 + 1, dtype=np.int64)
    t = np.flatnonzero(by_t)
    cnt[max_t - t] = by_t[t]                                # S / 2 = sum i^2 - T
    assert int(cnt.sum()) == math.factorial(n)
    cnt.setflags(write=False)
    _COUNTS[n] = cnt
    return cnt


def upper(n):
    """up[k] = P[S >= 2 k], k = 0 .. (n^3 - n) / 6: an integer suffix sum over n!, rounded once."""
    return np.cumsum(s_counts(n)[::-1])[::-1] / math.factorial(n)


def p_ge(n, s):
    """P[S >= s] for an even s."""
    assert s % 2 == 0
    if s <= 0:
        return 1.0
    return float(upper(n)[s // 2]) if s <= s_max(n) else 0.0


def p_le(n, s):
    """P[S <= s] for an even s (an integer prefix sum over n!, so small lower tails keep their digits)."""
    assert s % 2 == 0
    if s < 0:
        return 0.0
    return int(s_counts(n)[:s // 2 + 1].sum()) / math.factorial(n)


def pvalue(n, s, alternative):
    """cor.test's exact Spearman p-value at S = s: "greater" (rho > 0) is P[S <= s], "less" P[S >= s], "two.sided"
    twice the tail on s's side of the mean (n^3 - n) / 6, capped at 1."""
    if alternative == "greater":
        return p_le(n, s)
    if alternative == "less":
        return p_ge(n, s)
    assert alternative == "two.sided"
    return min(1.0, 2 * (p_ge(n, s) if s > (n ** 3 - n) / 6 else p_le(n, s)))


def s_of(perm):
    perm = np.asarray(perm, dtype=np.int64)
    return int(((np.arange(len(perm)) - perm) ** 2).sum())


def ladder(n, rng, min_distinct=40):
    """Permutations of 0 .. n - 1 whose S covers both tails and the centre: the identity, the reversal, from each of
    them n // 2 cumulative swaps of disjoint adjacent pairs (S moves by 2 per step), and 40 random ones.  Asserts
    that S in {0, 2, 4, S_max - 4, S_max - 2, S_max} are all there and at least ``min_distinct`` distinct S values
    (the callers with n < 10, where fewer exist or are likely, lower it)."""
    ident = np.arange(n)
    perms = [ident.copy(), ident[::-1].copy()]
    for start in (ident, ident[::-1]):
        cur = start.copy()
        for k in range(n // 2):
            cur = cur.copy()
            cur[2 * k], cur[2 * k + 1] = cur[2 * k + 1], cur[2 * k]
            perms.append(cur)
    perms += [rng.permutation(n) for _ in range(40)]
    s = {s_of(p) for p in perms}
    top = s_max(n)
    assert {0, 2, 4, top - 4, top - 2, top} <= s, sorted(s)
    assert len(s) >= min_distinct, len(s)
    return perms


# ---- cor_fast's Spearman pairs on ladder columns (any engine's cor_pairs: the device's, or api._cor_pairs_numpy) ----

ALTERNATIVES = ("two.sided", "less", "greater")


def ladder_matrix(n, pad=0, seed=6):
    """(X, S): column 0 holds 0 .. n - 1, column k the ladder's k-th permutation, so the pair (0, k) has S = S[k - 1]
    in integers.  Every column then gets an increasing affine map of its own to non-integers, and the rows are
    shuffled jointly.  pad > 0 appends rows where column 0 is NaN and the others hold arbitrary finite values: only
    pairwise deletion gives the n joint rows back.  The seed is one at which the 40 random permutations reach the
    series' worst stretch at every n the tests use, which assert_ladder_within_as89 asserts: about every other seed
    misses it (0.4 .. 0.6 x the table) at one n or another."""
    rng = np.random.default_rng(seed)
    perms = ladder(n, rng, min_distinct=40 if n >= 10 else 0)
    S = np.array([s_of(p) for p in perms], dtype=np.int64)
    X = np.column_stack([np.arange(n)] + perms).astype(np.float64)
    X = X * rng.uniform(0.3, 3.7, X.shape[1]) + rng.uniform(-9.5, 9.5, X.shape[1])
    if pad:
        extra = rng.normal(scale=20.0, size=(pad, X.shape[1]))
        extra[:, 0] = np.nan
        X = np.vstack([X, extra])
    return X[rng.permutation(X.shape[0])], S


def ladder_errors(cor_pairs, n, pad=0):
    """Runs pair (0, k) for every ladder column under each alternative (continuity off) and returns
    {alternative: worst error}: absolute for n >= 10, relative for the tabulated n <= 9.  Asserts what is exact: every
    reason 0 (ICIKT_COR_OK), n_values = n, rho = 1 - S / den within 1e-12."""
    X, S = ladder_matrix(n, pad)
    K = len(S)
    pi, pj = np.zeros(K, dtype=np.int32), np.arange(1, K + 1, dtype=np.int32)
    den = (n ** 3 - n) // 6
    worst = {}
    for alt in ALTERNATIVES:
        out, rsn = cor_pairs(X, pi, pj, "spearman", bool(pad), alt, False)
        assert not np.asarray(rsn).any(), (n, alt, np.asarray(rsn).tolist())
        assert np.array_equal(out[:, 2], np.full(K, float(n)))
        np.testing.assert_allclose(out[:, 0], 1.0 - S / den, atol=1e-12, rtol=0)
        want = np.array([pvalue(n, int(s), alt) for s in S])
        err = np.abs(out[:, 1] - want)
        worst[alt] = float((err if n >= 10 else err / want).max())
    return worst


def assert_ladder_within_as89(worst, n, label=""):
    """n >= 10: |p - exact| <= 1.25 x AS89_ERROR[n] one-sided, 2.5 x for "two.sided" (twice a tail), and, as a
    condition on the inputs, somewhere at least 0.6 x the table: the ladder does not sit where the series happens to
    be good.  n <= 9 (the tabulated distribution): 1e-12 relative."""
    print(f"{label} n = {n}: " + ", ".join(f"{a} {w:.4g}" for a, w in worst.items()))
    if n <= 9:
        assert max(worst.values()) <= 1e-12, (label, n, worst)
        return
    e = AS89_ERROR[n]
    assert worst["less"] <= 1.25 * e and worst["greater"] <= 1.25 * e and worst["two.sided"] <= 2.5 * e, (label, n, worst)
    assert max(worst["less"], worst["greater"], worst["two.sided"] / 2) >= 0.6 * e, (label, n, worst)


def factor_columns(n=1289, k=40, seed=7):
    """Tie-free columns for the large end of the Edgeworth range: column 0 is a factor f, column j = a_j f + noise with
    a_j spread over +-0.18, so that z = rho sqrt(n - 1) spans about -6 .. 6."""
    rng = np.random.default_rng(seed)
    f = rng.normal(size=n)
    a = np.linspace(-0.18, 0.18, k)
    X = np.column_stack([f] + [aj * f + math.sqrt(1 - aj * aj) * rng.normal(size=n) for aj in a])
    assert all(len(np.unique(X[:, j])) == n for j in range(X.shape[1]))
    return X
