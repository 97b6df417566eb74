"""The fast references of tests/diag_checker.py (column blocks sorted at once) against the per-column ones, scipy's
rankdata and np.median, and a few hand-worked rows: on CPU, no device."""
import math

import numpy as np
import pytest
import scipy.stats as st

from icikendalltau_amd import api
from tests import diag_checker as dc

GNAS = [dc.DEFAULT_NA, (), (math.nan,), (0.0,), (-0.0, math.inf), (math.nan, 3.0, -math.inf),
        tuple([math.nan] + [float(v) for v in range(31)])]


def _matrix(rng, n, S, model):
    if model == "lognormal":
        X = rng.lognormal(2, 1, size=(n, S))
        X[X < np.quantile(X, 0.2)] = np.nan if n * S else 0     # left-censored
    elif model == "ties":
        X = rng.integers(-3, 4, size=(n, S)).astype(np.float64)
    else:   # extremes
        X = rng.choice(np.array([np.inf, -np.inf, 0.0, -0.0, 1e300, -1e300, 1e-300, 1.7976931348623157e308,
                                 -1.7976931348623157e308, 2.5]), size=(n, S))
    X[rng.random((n, S)) < 0.15] = np.nan
    if n > 2 and S > 2:
        X[:, rng.integers(S)] = np.nan        # an all-missing column
        X[rng.integers(n), :] = np.nan        # an all-missing row
    return np.asfortranarray(X)


CASES = [(n, S, model, seed) for seed, (n, S) in enumerate([(1, 1), (1, 4), (2, 3), (3, 5), (7, 6), (8, 9), (33, 12),
                                                             (64, 3), (101, 20)])
         for model in ("lognormal", "ties", "extremes")]


@pytest.mark.parametrize("n,S,model,seed", CASES)
def test_fast_references_match_slow(n, S, model, seed):
    rng = np.random.default_rng(seed * 7 + len(model))
    X = _matrix(rng, n, S, model)
    for gna in GNAS:
        miss, _ex = dc.rule(X, gna)
        for na_rm in (False, True):
            np.testing.assert_array_equal(dc.ref_col_medians(X, miss, na_rm), dc.ref_col_medians_slow(X, miss, na_rm))
        cls = rng.integers(0, 4, size=S)
        fast, slow = dc.ref_censor(X, gna, cls, 5), dc.ref_censor_slow(X, gna, cls, 5)
        for a, b in zip(fast[:3], slow[:3]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(dc.bits(fast[3]), dc.bits(slow[3]))
        for cols in (np.arange(S), rng.permutation(S)[: max(1, S // 2)]):
            f, s = dc.ref_rank_order(X, gna, cols), dc.ref_rank_order_slow(X, gna, cols)
            assert f["n_kept"] == s["n_kept"]
            for key in ("n_na", "row_order", "col_order", "ranks"):
                np.testing.assert_array_equal(f[key], s[key], err_msg=key)
            for key in ("median_rank", "original", "ordered"):
                np.testing.assert_array_equal(dc.bits(f[key]), dc.bits(s[key]), err_msg=key)


@pytest.mark.parametrize("seed", range(6))
def test_doubled_ranks_match_rankdata_and_median(seed):
    rng = np.random.default_rng(100 + seed)
    n, m = int(rng.integers(1, 60)), int(rng.integers(1, 9))
    V = _matrix(rng, n, m, ("lognormal", "ties", "extremes")[seed % 3])
    mk = np.isnan(V) | (rng.random(V.shape) < 0.1)
    r2 = dc.doubled_ranks(V, mk)
    for j in range(m):
        k = int(mk[:, j].sum())
        want = np.zeros(n)
        want[mk[:, j]] = np.arange(1, k + 1)
        if k < n:
            want[~mk[:, j]] = k + st.rankdata(V[~mk[:, j], j], method="average")
        np.testing.assert_array_equal(r2[:, j], 2 * want)
    assert (r2 < 2 ** 20).all()
    np.testing.assert_array_equal(np.median(r2, axis=1) / 2, np.median(r2 / 2, axis=1))


def test_hand_worked_rows():
    # column 0: 3, NaN, 1, 1, 0 with global_na 0 -> missing rows 1 and 4 take ranks 1, 2, the two 1s tie at 3.5, 3 is 5;
    # column 1 ranks 1 .. 5; row medians 3, 1.5, 3.25, 3.75, 3.5
    X = np.array([[3.0, 1.0], [np.nan, 2.0], [1.0, 3.0], [1.0, 4.0], [0.0, 5.0]], order="F")
    r = dc.ref_rank_order(X, (0.0,), [0, 1])
    np.testing.assert_array_equal(r["ranks"][:, 0], [5, 1, 3.5, 3.5, 2])
    np.testing.assert_array_equal(r["median_rank"], [3, 1.5, 3.25, 3.75, 3.5])
    np.testing.assert_array_equal(r["row_order"], [3, 4, 2, 0, 1])
    np.testing.assert_array_equal(r["col_order"], [0, 1])
    # one column: rows missing in every column of the class are dropped before ranking
    r = dc.ref_rank_order(X, (0.0,), [0])
    assert r["n_kept"] == 3
    np.testing.assert_array_equal(r["median_rank"][[0, 2, 3]], [3, 1.5, 1.5])
    # a row across four columns: doubled ranks 2, 7, 8, 8 -> median (7 + 8) / 4 = 3.75
    X = np.array([[1.0, 5.0, 1.0, 2.0],
                  [2.0, 5.0, 9.0, 9.0],
                  [3.0, 1.0, 2.0, 3.0],
                  [4.0, 2.0, 3.0, 1.0]], order="F")
    r = dc.ref_rank_order(X, (), np.arange(4))
    np.testing.assert_array_equal(r["ranks"][0], [1, 3.5, 1, 2])
    assert r["median_rank"][0] == 1.5
    np.testing.assert_array_equal(r["ranks"][1], [2, 3.5, 4, 4])
    assert r["median_rank"][1] == 3.75
    # medians: -Inf and Inf -> NaN bits; two maxima -> the finite 0.5 a + 0.5 b; a lone -0 -> +0; empty -> NA
    X = np.array([[-np.inf, 1.7976931348623157e308, -0.0, np.nan],
                  [np.inf, 1.7976931348623157e308, np.nan, np.nan]], order="F")
    got = dc.ref_col_medians(X, np.isnan(X), True)
    assert got.tolist() == [int(dc.NAN_BITS), int(dc.bits(1.7976931348623157e308)[()]), 0, int(dc.NA_BITS)]
    assert dc.ref_col_medians(X, np.isnan(X), False)[2] == dc.NA_BITS
    # censor: class 0 = columns 0, 1; rows 1 and 2 have a missing cell; medians 2 and 20
    X = np.array([[1.0, 10.0], [2.0, np.nan], [np.nan, 30.0], [4.0, 20.0]], order="F")
    tr, su, nex, _med = dc.ref_censor(X, (math.nan,), np.array([0, 0]), 2)
    assert tr.tolist() == [2, 0] and su.tolist() == [0, 0] and nex == 2


@pytest.mark.parametrize("n,S", [(300, 70), (1200, 9)])
def test_numpy_front_end_path_matches(n, S):
    """The library's own engine-free numpy path (api._*_numpy) and the fast references agree on the same inputs."""
    rng = np.random.default_rng(n + S)
    X = _matrix(rng, n, S, "ties")
    gna = list(dc.DEFAULT_NA)
    for na_rm in (False, True):
        np.testing.assert_array_equal(dc.bits(api._col_medians_numpy(X, na_rm)),
                                      dc.ref_col_medians(X, np.isnan(X), na_rm))
    cls = rng.integers(0, 5, size=S)
    tr, su, nex = api._censor_numpy(X, gna, cls, 6)
    rtr, rsu, rnex, _ = dc.ref_censor(X, dc.DEFAULT_NA, cls, 6)
    assert tr.tolist() == rtr.tolist() and su.tolist() == rsu.tolist() and nex == rnex
    cols = np.flatnonzero(cls == 2).astype(np.int32)
    dc.assert_rank_order(api._rank_order_numpy(X, gna, cols), X, dc.DEFAULT_NA, cols)


def test_sweep_cases_on_numpy_path(tmp_path, monkeypatch):
    """A few cases of the GPU sweep's generator (tests/diag_cor_cases.py) through the engine-free numpy diagnostics."""
    from tests import diag_cor_cases
    from tests.numpy_ctx import NumpyCtx

    monkeypatch.setattr(diag_cor_cases, "LENGTHS", [1, 2, 3, 63, 64, 65, 255, 256, 257])
    rng = np.random.default_rng(5)
    bad = [m for case in range(12) if (m := diag_cor_cases.one_case(NumpyCtx(), rng, case, str(tmp_path), cor=False))]
    assert not bad, "\n".join(bad)
