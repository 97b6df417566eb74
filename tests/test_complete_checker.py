"""tests/complete_checker.py pinned independently of the oracle's own missing-value handling: for seeded pairs the
incomplete rows are ACTUALLY dropped, and what the checker answers for the masked columns must be scipy's tau-b and the
O(n^2) enumeration's counts of the dropped vectors.  (The device test compares with the checker: without this it would
be the oracle against the oracle's "local" perspective.)"""
import warnings

import numpy as np
from scipy import stats

from oracle import oracle as O
from tests import complete_checker as cc


def test_checker_equals_scipy_and_enumeration_on_dropped_rows():
    rng = np.random.default_rng(20240)
    seen = {0: 0, 1: 0, 2: 0, 3: 0}
    two_rows = inf_pairs = total = 0
    for n in (1, 2, 3, 4, 7, 20, 41, 60):
        X = cc.degenerate_columns(rng, n)
        S = X.shape[1]
        pi, pj = (a.astype(np.int32) for a in np.triu_indices(S, k=0))     # self pairs too
        out, cnt, rsn = cc.check_pairs_complete(X, pi, pj)
        Xp = cc.masked(X, pi, pj)
        assert Xp.shape == (n, 2 * len(pi)) and Xp.flags.f_contiguous
        for k, (i, j) in enumerate(zip(pi, pj)):
            keep = ~(np.isnan(X[:, i]) | np.isnan(X[:, j]))
            x, y = X[keep, i], X[keep, j]
            m = int(keep.sum())
            assert np.array_equal(Xp[keep, 2 * k], x) and np.array_equal(Xp[keep, 2 * k + 1], y)
            assert np.isnan(Xp[~keep, 2 * k:2 * k + 2]).all()
            total += 1
            r = int(rsn[k])
            # the reasons the reference gives: nothing left, fewer than two rows, a constant side
            want = 1 if m == 0 else 2 if m < 2 else 3 if (len(np.unique(x)) == 1 or len(np.unique(y)) == 1) else 0
            assert r == want, (n, i, j, m, r)
            seen[r] += 1
            if r != 0:
                assert np.isnan(out[k, 0]) and np.isnan(out[k, 1])
                continue
            c = dict(zip(O.COUNT_FIELDS, cnt[k].tolist()))
            assert c["n"] == m and c["missing"] == 0, (n, i, j, c)
            bf = O.bruteforce(x, y, "local")
            assert (c["dis"], c["ntie"], c["xtie"], c["ytie"]) == (bf["dis"], bf["ntie"], bf["xtie"], bf["ytie"]), (n, i, j)
            assert c["tot"] == m * (m - 1) // 2 == bf["con"] + bf["dis"] + bf["xtie"] + bf["ytie"] - bf["ntie"]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                tau = stats.kendalltau(x, y, variant="b").statistic
            assert abs(out[k, 0] - tau) <= 1e-12, (n, i, j, out[k, 0], tau)
            two_rows += m == 2
            inf_pairs += bool(np.isinf(x).any() or np.isinf(y).any())
    assert total >= 800 and min(seen.values()) >= 8, seen       # every degenerate kind, and healthy pairs between them
    assert two_rows >= 3 and inf_pairs >= 100, (two_rows, inf_pairs)


def test_two_joint_rows_have_a_tau_and_no_p_value():
    """Two joint rows: reason 0, tau = +-1, p-value NaN (a variance of zero) -- what the device must reproduce."""
    X = np.array([[1.0, 5.0, 2.0], [np.nan, 1.0, np.nan], [2.0, 4.0, 3.0], [np.nan, np.nan, 9.0]], order="F")
    out, cnt, rsn = cc.check_pairs_complete(X, [0, 0], [1, 2])
    assert rsn.tolist() == [0, 0] and out[:, 0].tolist() == [-1.0, 1.0] and np.isnan(out[:, 1]).all()
    assert cnt[:, 0].tolist() == [2, 2] and cnt[:, 1].tolist() == [0, 0]
    # a list that repeats pairs is answered per entry, in the list's order
    out3, cnt3, rsn3 = cc.check_pairs_complete(X, [0, 2, 0, 0], [2, 0, 1, 2])
    assert np.array_equal(out3[[2, 0]], out, equal_nan=True) and np.array_equal(out3[3], out3[0], equal_nan=True)
    assert np.array_equal(cnt3[[2, 0]], cnt) and np.array_equal(cnt3[1, [4, 5]], cnt3[0, [5, 4]])      # xtie / ytie swap
