"""The missing-value diagnostics on the MI355X (icikt_col_medians_f64, icikt_censor_counts_f64, icikt_rank_order_f64)
against an independent restatement (tests/diag_checker.py): numpy's sort for the medians, one sort per column block for
the ranks (pinned to scipy's rankdata), numpy's stable argsort for the orders.  Every comparison is exact: medians and
copied cells bit for bit, counts, ranks and orders equal."""
import math
import os

import numpy as np
import pytest

import icikendalltau_amd as ik
from icikendalltau_amd import _lib
from tests.diag_checker import DEFAULT_NA, NA_BITS, bits, ref_col_medians, ref_censor, ref_rank_order, rule

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def check_medians(ctx, X, na_rm):
    got = bits(ctx.col_medians(X, na_rm))
    np.testing.assert_array_equal(got, ref_col_medians(X, np.isnan(X), na_rm))


def check_censor(ctx, X, gna, cls=None):
    cls = np.zeros(X.shape[1], np.int32) if cls is None else np.asarray(cls, np.int32)
    n_class = int(cls.max()) + 1
    tr, su, nex, med = ctx.censor_counts(X, gna, cls, n_class, want_medians=True)
    rtr, rsu, rnex, rmed = ref_censor(X, gna, cls, n_class)
    np.testing.assert_array_equal(tr, rtr)
    np.testing.assert_array_equal(su, rsu)
    assert nex == rnex
    np.testing.assert_array_equal(bits(med), ref_col_medians(X, rule(X, gna)[0], True))


def check_rank(ctx, X, gna, cols=None):
    cols = np.arange(X.shape[1], dtype=np.int32) if cols is None else np.asarray(cols, np.int32)
    got = ctx.rank_order(X, gna, cols)
    ref = ref_rank_order(X, gna, cols)
    assert got["n_kept"] == ref["n_kept"]
    np.testing.assert_array_equal(got["n_na"], ref["n_na"])
    np.testing.assert_array_equal(bits(got["median_rank"])[ref["n_na"] < len(cols)],
                                  bits(ref["median_rank"])[ref["n_na"] < len(cols)])
    assert (bits(got["median_rank"])[ref["n_na"] == len(cols)] == NA_BITS).all()
    np.testing.assert_array_equal(got["row_order"], ref["row_order"])
    np.testing.assert_array_equal(got["col_order"], ref["col_order"])
    np.testing.assert_array_equal(bits(got["original"]), bits(ref["original"]))
    np.testing.assert_array_equal(bits(got["ordered"]), bits(ref["ordered"]))
    return got


def censored(rng, n, S, frac=0.2, ties=False):
    X = rng.integers(0, 7, size=(n, S)).astype(np.float64) if ties else rng.lognormal(3, 1, size=(n, S))
    X[rng.random((n, S)) < frac] = np.nan
    X[rng.random((n, S)) < 0.05] = 0.0
    return np.asfortranarray(X)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 64, 255, 256, 257, 1000, 2049])
def test_small_and_odd_even_rows(ctx, n):
    rng = np.random.default_rng(n)
    X = censored(rng, n, 5)
    for na_rm in (False, True):
        check_medians(ctx, X, na_rm)
    check_censor(ctx, X, DEFAULT_NA)
    check_rank(ctx, X, DEFAULT_NA)
    check_rank(ctx, X[:, :1].copy(order="F"), DEFAULT_NA)


def test_all_missing_rows_and_columns(ctx):
    rng = np.random.default_rng(1)
    X = censored(rng, 300, 7)
    X[:, 2] = np.nan
    X[10:40, :] = np.nan
    X[50, :] = 0.0
    for na_rm in (False, True):
        check_medians(ctx, X, na_rm)
    check_censor(ctx, X, DEFAULT_NA)
    check_rank(ctx, X, DEFAULT_NA)
    check_rank(ctx, np.full((20, 3), np.nan, order="F"), DEFAULT_NA)


def test_heavy_ties(ctx):
    rng = np.random.default_rng(2)
    X = censored(rng, 5000, 12, frac=0.3, ties=True)
    check_medians(ctx, X, True)
    check_censor(ctx, X, DEFAULT_NA, cls=np.arange(12) % 3)
    check_rank(ctx, X, DEFAULT_NA)
    check_rank(ctx, X, (math.nan,))


def test_infinities_zeros_and_extremes(ctx):
    rng = np.random.default_rng(3)
    X = censored(rng, 401, 9)
    X[rng.random(X.shape) < 0.05] = np.inf
    X[rng.random(X.shape) < 0.05] = -np.inf
    X[rng.random(X.shape) < 0.05] = -0.0
    X[:, 3] = np.where(np.arange(401) % 2, 1.7e308, -1.7e308)
    X[:200, 4] = -np.inf       # the middle of column 4 pairs -Inf with +Inf: NaN median
    X[200:, 4] = np.inf
    X[:, 5] = np.where(np.arange(401) < 200, 1.7976931348623157e308, 1.797693134862315e308)
    X[:, 6] = -0.0
    X[:, 6][::3] = 0.0
    Xe = X[:400].copy(order="F")   # even row count: the midpoints
    for A in (X, Xe):
        for na_rm in (False, True):
            check_medians(ctx, A, na_rm)
        for gna in (DEFAULT_NA, (math.nan, 0.0), (math.nan,), (0.0,), (), (-0.0, 1.7e308)):
            check_censor(ctx, A, gna)
            check_rank(ctx, A, gna)


def test_seventeen_interleaved_classes(ctx):
    rng = np.random.default_rng(4)
    S = 17 * 5 + 6
    X = censored(rng, 777, S)
    cls = rng.integers(0, 17, size=S)
    cls[:17] = np.arange(17)
    check_censor(ctx, X, DEFAULT_NA, cls=cls)
    for k in range(17):
        check_rank(ctx, X, DEFAULT_NA, np.flatnonzero(cls == k))
    res = ik.rank_order_data(X, sample_classes=[f"c{k:02d}" for k in cls])
    assert list(res) == [f"c{k:02d}" for k in range(17)]


def test_many_global_na_values_host_mask(ctx):
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.integers(0, 60, size=(500, 8)).astype(np.float64))
    X[rng.random(X.shape) < 0.1] = np.nan
    gna = [math.nan] + [float(v) for v in range(40)]
    with pytest.raises(_lib.IciktError, match="more than 32"):
        ctx.rank_order(X, gna, np.arange(8, dtype=np.int32))
    miss, ex = rule(X, gna)
    cpu = ik.test_left_censorship(X, global_na=gna, engine=object())
    gpu = ik.test_left_censorship(X, global_na=gna)
    assert gpu["values"].equals(cpu["values"])
    assert gpu["binomial_test"] == cpu["binomial_test"]
    r_cpu = ik.rank_order_data(X, global_na=gna, engine=object())
    r_gpu = ik.rank_order_data(X, global_na=gna)
    np.testing.assert_array_equal(bits(r_gpu["ordered"].to_numpy()), bits(r_cpu["ordered"].to_numpy()))
    np.testing.assert_array_equal(r_gpu["row_order"], r_cpu["row_order"])


def test_non_contiguous_input_and_leading_dimension(ctx):
    rng = np.random.default_rng(6)
    big = censored(rng, 700, 10)
    X = big[::2, ::2]          # neither C- nor F-contiguous
    check_rank(ctx, np.asfortranarray(X), DEFAULT_NA)
    a = ik.rank_order_data(X)
    b = ik.rank_order_data(np.ascontiguousarray(X))
    np.testing.assert_array_equal(bits(a["ordered"].to_numpy()), bits(b["ordered"].to_numpy()))
    # ld > n_feat through the C entry: the first 300 of 700 rows
    got = ctx.rank_order(big, DEFAULT_NA, np.array([1, 4, 7], np.int32), n_feat=300)
    ref = ref_rank_order(np.asfortranarray(big[:300]), DEFAULT_NA, np.array([1, 4, 7]))
    np.testing.assert_array_equal(got["row_order"], ref["row_order"])
    np.testing.assert_array_equal(bits(got["ordered"]), bits(ref["ordered"]))


@pytest.mark.parametrize("n", [65535, 65536, 65537, 262144])
def test_long_columns(ctx, n):
    rng = np.random.default_rng(n)
    X = censored(rng, n, 3, ties=n == 65536)
    check_medians(ctx, X, True)
    check_censor(ctx, X, DEFAULT_NA, cls=[0, 1, 0])
    check_rank(ctx, X, DEFAULT_NA)


def test_too_long(ctx):
    X = np.zeros((262145, 2), order="F")
    for call in (lambda: ctx.col_medians(X), lambda: ctx.censor_counts(X, DEFAULT_NA, [0, 0], 1),
                 lambda: ctx.rank_order(X, DEFAULT_NA, [0, 1])):
        with pytest.raises(_lib.IciktError, match="ICIKT_MAX_FEATURES_WIDE"):
            call()


def test_known_answers_on_device():
    X = np.load(os.path.join(GOLDEN, "missing_dataset.npz"))["X"]
    r = ik.test_left_censorship(X)
    assert r["values"]["trials"].tolist() == [1900] and r["values"]["success"].tolist() == [1520]
    assert r["binomial_test"]["p_value"] == pytest.approx(2.7471901850880075e-161, rel=1e-12)
    Y = np.load(os.path.join(GOLDEN, "yeast_missing.npz"))["X"]
    r = ik.test_left_censorship(Y, sample_classes=["snf2"] * 48 + ["wt"] * 48)
    assert r["values"]["trials"].tolist() == [18336, 20424]
    assert r["values"]["success"].tolist() == [18336, 20424]
    assert r["binomial_test"]["conf_int"][0] == pytest.approx(0.05 ** (1 / 38760), rel=1e-14)


def test_front_ends_match_numpy_path():
    rng = np.random.default_rng(7)
    X = censored(rng, 999, 11)
    cls = ["b", "a"] * 5 + ["c"]
    for use in ("col", "row"):
        for na_rm in (False, True):
            np.testing.assert_array_equal(bits(ik.calculate_matrix_medians(X, use, na_rm)),
                                          bits(ik.calculate_matrix_medians(X, use, na_rm, engine=object())))
    a = ik.test_left_censorship(X, sample_classes=cls)
    b = ik.test_left_censorship(X, sample_classes=cls, engine=object())
    assert a["values"].equals(b["values"]) and a["binomial_test"] == b["binomial_test"]
    ra = ik.rank_order_data(X, sample_classes=cls)
    rb = ik.rank_order_data(X, sample_classes=cls, engine=object())
    for k in ("a", "b", "c"):
        for part in ("original", "ordered", "n_na_rank"):
            assert ra[k][part].equals(rb[k][part]) or np.array_equal(
                bits(ra[k][part].to_numpy(dtype=np.float64)), bits(rb[k][part].to_numpy(dtype=np.float64)))
        np.testing.assert_array_equal(ra[k]["row_order"], rb[k]["row_order"])
