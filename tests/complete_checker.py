"""Reference for icikt_pairs_complete_f64 / _in (kt_fast use = "pairwise.complete.obs"), test infrastructure only.

The entry is specified to build, per pair k of the list, two columns (2k, 2k+1): the pair's columns with BOTH entries of
every row that misses either value set missing; and to answer ici_kt(..., perspective = "local") of those two.  `masked`
builds that matrix on the host, `check_pairs_complete` runs the CPU oracle over it.  tests/test_complete_checker.py pins
this against scipy and the O(n^2) enumeration on vectors whose rows are actually dropped."""
import numpy as np

from oracle import oracle as O

NA_BITS = np.uint64(0x7FF00000000007A2)      # R's NA_real_: what a pair without a result carries
ATOL = 1e-10                                 # BASELINE.json north_star: the four doubles


def masked(X, pi, pj):
    """The n x 2P column-major matrix of the masked column pairs."""
    X = np.asarray(X, dtype=np.float64)
    pi, pj = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64)
    n, P = X.shape[0], len(pi)
    Xp = np.empty((n, 2 * P), dtype=np.float64, order="F")
    step = max(1, (1 << 24) // max(n, 1))
    for b in range(0, P, step):
        i, j = pi[b:b + step], pj[b:b + step]
        a, c = X[:, i], X[:, j]
        either = np.isnan(a) | np.isnan(c)
        Xp[:, 2 * b:2 * (b + len(i)):2] = np.where(either, np.nan, a)
        Xp[:, 2 * b + 1:2 * (b + len(i)):2] = np.where(either, np.nan, c)
    return Xp


def check_pairs_complete(X, pi, pj, alternative="two.sided", continuity=False, int32_compat=True):
    """(out4 [P, 4], counts [P, 12], reasons [P]) of the pairs (pi[k], pj[k]) with their incomplete rows dropped: the
    oracle's "local" answer for columns (2k, 2k+1) of masked(X, pi, pj).  A list that repeats pairs (the device tests'
    lists over a few dozen columns) is masked and run once per distinct ordered pair."""
    pi, pj = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64)
    S = np.asarray(X).shape[1]
    key, inv = np.unique(pi * S + pj, return_inverse=True)
    ui, uj = key // S, key % S
    k = np.arange(len(key), dtype=np.int32)
    out, cnt, rsn = O.ici_pairs(masked(X, ui, uj), 2 * k, 2 * k + 1, "local", alternative, continuity,
                                int32_compat=int32_compat)
    return out[inv], cnt[inv], rsn[inv]


def degenerate_columns(rng, n):
    """16 columns of n rows whose pairs lose their rows in every way: 0 .. 7 continuous, tied and +-Inf with 20 % NaN;
    8 constant; 9 constant where present; 10 all NaN; 11 / 12 disjoint presence; 13 one row present; 14 two rows
    present; 15 most rows missing."""
    X = rng.standard_normal((n, 16))
    X[:, 2] = np.round(X[:, 2] * 2)
    X[:, 3] = rng.integers(0, 3, n)
    X[:, 4] = np.where(rng.random(n) < 0.2, np.inf, X[:, 4])
    X[:, 5] = np.where(rng.random(n) < 0.2, -np.inf, np.round(X[:, 5]))
    X[:, 6] = np.where(rng.random(n) < 0.15, np.inf, np.where(rng.random(n) < 0.15, -np.inf, X[:, 6]))
    X[:, :8][rng.random((n, 8)) < 0.2] = np.nan
    X[:, 8] = 2.5
    X[:, 9] = np.where(rng.random(n) < 0.5, np.nan, -1.0)
    X[:, 10] = np.nan
    half = rng.permutation(n) < n // 2
    X[:, 11] = np.where(half, X[:, 11], np.nan)
    X[:, 12] = np.where(half, np.nan, X[:, 12])
    rows = rng.permutation(n)
    X[:, 13] = np.where(np.isin(np.arange(n), rows[:1]), X[:, 13], np.nan)
    X[:, 14] = np.where(np.isin(np.arange(n), rows[:2]), X[:, 14], np.nan)
    X[:, 15] = np.where(rng.random(n) < 0.7, np.nan, X[:, 15])
    return np.asfortranarray(X)


def assert_complete(got, ref, label="", sel=None):
    """The suite's comparison: reasons equal, counts bit-exact where the reason is 0, the NaN pattern equal with the NA
    payload on failed pairs, doubles within 1e-10.  got: (out4, counts or None, reasons or None) of all pairs; ref: the
    checker's answer for the pairs `sel` (None: all)."""
    out, cnt, rsn = got
    rout, rcnt, rrsn = ref
    if sel is not None:
        out = out[sel]
        cnt = None if cnt is None else cnt[sel]
        rsn = None if rsn is None else rsn[sel]
    ok = rrsn == 0
    if rsn is not None:
        bad = np.flatnonzero(rsn != rrsn)
        assert len(bad) == 0, f"{label} reasons: pairs {bad[:8].tolist()}: {rsn[bad[:8]].tolist()} != {rrsn[bad[:8]].tolist()}"
    if cnt is not None:
        bad = np.flatnonzero(np.any(cnt != rcnt[:, :cnt.shape[1]], axis=1) & ok)
        assert len(bad) == 0, f"{label} counts: pairs {bad[:8].tolist()}: {cnt[bad[0]].tolist()} != {rcnt[bad[0]].tolist()}"
    nan_g, nan_r = np.isnan(out), np.isnan(rout)
    bad = np.flatnonzero(np.any(nan_g != nan_r, axis=1))
    assert len(bad) == 0, f"{label} NaN pattern: pairs {bad[:8].tolist()}: {out[bad[0]].tolist()} != {rout[bad[0]].tolist()}"
    both = ~nan_r
    d = np.abs(np.where(both, out, 0.0) - np.where(both, rout, 0.0))
    assert d.max(initial=0.0) <= ATOL, f"{label} doubles: pair {int(np.argmax(d.max(axis=1)))}, |d| = {d.max()!r}"
    failed = ~ok & np.isnan(rout[:, 0])
    bits = np.ascontiguousarray(out).view(np.uint64)
    assert np.all(bits[failed][np.isnan(out[failed])] == NA_BITS), f"{label}: failed pairs without the NA payload"
