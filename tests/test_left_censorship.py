"""test_left_censorship, calculate_matrix_medians and rank_order_data through their numpy path (an engine without the
device methods), and the package's binomial helpers.

tests/golden/missing_dataset.npz is the reference's data/missing_dataset.rda (1000 x 20, 100 NA, no dimnames), read
once with icikendalltau_amd.formats.read_r_matrix and saved as X.  Expected values: the reference's vignette and
testthat file; the p-value from scipy.stats.binomtest.
"""
import math
import os

import numpy as np
import pytest
import scipy.stats as st

import icikendalltau_amd as ik
from icikendalltau_amd import api
from oracle.rrng import RRandom

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CPU = object()   # an engine without col_medians / censor_counts / rank_order: the numpy path


def _missing_dataset():
    return np.load(os.path.join(GOLDEN, "missing_dataset.npz"))["X"]


def test_missing_dataset_known_answer():
    r = ik.test_left_censorship(_missing_dataset(), engine=CPU)
    v = r["values"]
    assert v["trials"].tolist() == [1900] and v["success"].tolist() == [1520] and v["class"].tolist() == ["A"]
    b = r["binomial_test"]
    assert b["p_value"] == pytest.approx(2.7471901850880075e-161, rel=1e-12)
    assert b["conf_int"][0] == pytest.approx(0.7843033190664356, rel=1e-14)
    assert round(b["conf_int"][0], 7) == 0.7843033 and b["conf_int"][1] == 1.0
    assert b["estimate"] == 0.8 and b["null_value"] == 0.5
    assert (b["statistic"], b["parameter"]) == (1520, 1900)
    assert b["statistic_name"] == "number of successes" and b["parameter_name"] == "number of trials"
    assert b["method"] == "Exact binomial test" and b["data_name"] == "total_success and total_trials"
    assert b["alternative"] == "greater"


def test_yeast_two_classes_known_answer():
    X = np.load(os.path.join(GOLDEN, "yeast_missing.npz"))["X"]
    r = ik.test_left_censorship(X, sample_classes=["snf2"] * 48 + ["wt"] * 48, engine=CPU)
    v = r["values"]
    assert v["class"].tolist() == ["snf2", "wt"]
    assert v["trials"].tolist() == [18336, 20424] and v["success"].tolist() == [18336, 20424]
    b = r["binomial_test"]
    assert b["conf_int"][0] == pytest.approx(0.05 ** (1 / 38760), rel=1e-14)
    assert round(b["conf_int"][0], 7) == 0.9999227
    assert b["p_value"] == 0.0 and b["estimate"] == 1.0


def _reference_testthat_data():
    """The data of the reference's tests/testthat/test-left_censorship.R, each withr::with_seed(1234, ...) restated."""
    n_feature, n_sample, n_miss, n_low = 1000, 20, 100, 80
    test_dataset = np.sort(np.exp(RRandom(1234).rnorm(n_feature, 10, 1)))
    noise = RRandom(1234).rnorm(n_feature * n_sample, 0, 0.1).reshape((n_feature, n_sample), order="F")
    noisy = np.log(test_dataset)[:, None] + noise
    low = RRandom(1234).sample(300, n_low)
    hi = 799 + RRandom(1234).sample(201, n_miss - n_low)
    all_idx = np.concatenate([low, hi]) - 1
    rng = RRandom(1234)
    samp = np.array([rng.unif_index(n_sample) + 1 for _ in range(n_miss)]) - 1
    rng = RRandom(1234)
    group_samp = np.array([rng.unif_index(n_sample // 2) + 1 for _ in range(n_miss)]) - 1
    return noisy, all_idx, samp, group_samp, n_low / n_miss


def test_reference_testthat_file(capsys):
    noisy, all_idx, samp, group_samp, ratio = _reference_testthat_data()
    assert ik.test_left_censorship(noisy, engine=CPU) is None
    assert "has no missing values" in capsys.readouterr().out
    zero = noisy.copy()
    zero[all_idx, samp] = 0
    zero_binom = ik.test_left_censorship(zero, global_na=(0, math.nan), engine=CPU)
    v = zero_binom["values"]
    assert v["success"][0] / v["trials"][0] == pytest.approx(ratio)
    assert (v["trials"][0], v["success"][0]) == (1900, 1520)
    na = zero.copy()
    na[zero == 0] = np.nan
    na_binom = ik.test_left_censorship(na, global_na=(0, math.nan), engine=CPU)
    assert na_binom["values"]["success"][0] / na_binom["values"]["trials"][0] == pytest.approx(ratio)
    assert na_binom["values"].equals(zero_binom["values"])
    assert na_binom["binomial_test"] == zero_binom["binomial_test"]
    na_loc = np.flatnonzero(np.isnan(na).ravel(order="F"))
    back_zero = na_loc[RRandom(1234).sample(na_loc.size, 20) - 1]
    mix = na.copy(order="F")
    mix.ravel(order="K")[back_zero] = 0
    assert (mix == 0).sum() == 20
    mix_binom = ik.test_left_censorship(mix, global_na=(0, math.nan), engine=CPU)
    assert mix_binom["values"].equals(na_binom["values"])
    assert mix_binom["binomial_test"] == na_binom["binomial_test"]
    group = noisy.copy()
    group[all_idx, group_samp] = 0
    g = ik.test_left_censorship(group, sample_classes=["A"] * 10 + ["B"] * 10, engine=CPU)
    assert len(g["values"]) == 2
    assert g["values"]["success"][0] / g["values"]["trials"][0] == pytest.approx(ratio)


@pytest.mark.parametrize("x, n", [(0, 1), (1, 1), (0, 7), (7, 7), (3, 10), (1000, 1900), (1520, 1900), (18336, 18336),
                                  (500_000, 1_000_000), (5_020_000, 10_000_000), (2_000_000, 3_000_000)])
def test_pbinom_qbeta_against_scipy(x, n):
    p = api.pbinom_upper(x, n)
    ref = st.binom.sf(x - 1, n, 0.5)
    assert p == pytest.approx(ref, rel=1e-11, abs=1e-300)
    if x > 0:
        assert api.qbeta_binom_lower(0.05, x, n) == pytest.approx(st.beta.ppf(0.05, x, n - x + 1), rel=1e-12)


def test_pbinom_qbeta_near_two_to_the_31():
    n = 2 ** 31 - 1
    for k in (-3, 0.5, 3, 30):
        x = int(n / 2 + k * math.sqrt(n) / 2)
        # scipy's own tail is off by ~4e-8 relative at this n; the independent check below is tighter
        assert api.pbinom_upper(x, n) == pytest.approx(st.binom.sf(x - 1, n, 0.5), rel=1e-7)
        assert api.qbeta_binom_lower(0.05, x, n) == pytest.approx(st.beta.ppf(0.05, x, n - x + 1), rel=1e-11)
    assert api.pbinom_upper(n, n) == 0.0 and api.pbinom_upper(0, n) == 1.0
    assert api.qbeta_binom_lower(0.05, n, n) == pytest.approx(0.05 ** (1 / n), rel=1e-14)


def test_pbinom_tail_against_exact_sum():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 30
    n = 2 ** 31 - 1
    x = int(n / 2 + 15 * math.sqrt(n))
    t = mp.exp(mp.loggamma(n + 1) - mp.loggamma(x + 1) - mp.loggamma(n - x + 1) - n * mp.log(2))
    s, j = mp.mpf(0), x
    while t > s * mp.mpf(10) ** -25:
        s += t
        t = t * (n - j) / (j + 1)
        j += 1
    assert api.pbinom_upper(x, n) == pytest.approx(float(s), rel=1e-11)


def test_n_zero_error_and_message(capsys):
    X = np.array([[1.0, 2.0], [np.nan, np.nan]])
    with pytest.raises(ValueError, match="^'n' must be a positive integer >= 'x'$"):
        ik.test_left_censorship(X, engine=CPU)
    assert ik.test_left_censorship(np.ones((3, 2)), engine=CPU) is None
    assert capsys.readouterr().out == "i `data_matrix` has no missing values, returning NULL\n"
    with pytest.raises(TypeError, match="must be a numeric type"):
        ik.test_left_censorship(np.array([["a", "b"]]), engine=CPU)


def test_nan_outside_global_na_is_missing_but_no_early_return(capsys):
    X = np.array([[1.0, 2.0, 3.0], [np.nan, 5.0, 0.0], [4.0, 6.0, 7.0]])
    assert ik.test_left_censorship(X, global_na=(math.inf,), engine=CPU) is None   # the rule's mask alone
    r = ik.test_left_censorship(X, global_na=(0,), engine=CPU)
    # row 2 has two missing cells (NaN, 0); its one value 5 is compared with column 2's median 5: a trial, no success
    assert (r["values"]["trials"][0], r["values"]["success"][0]) == (1, 0)


def test_class_order():
    levels, cls = api._class_levels([10, 2, 10, 1], 4, "A")
    assert levels == [1, 2, 10] and cls.tolist() == [2, 1, 2, 0]
    levels, cls = api._class_levels(["wt", "b", "B", "a"], 4, "A")
    assert levels == ["B", "a", "b", "wt"]
    X = np.array([[np.nan, 1.0, 2.0, 0.0], [3.0, 4.0, 5.0, 6.0]])
    r = ik.test_left_censorship(X, sample_classes=["z", "y", "z", "y"], engine=CPU)
    assert r["values"]["class"].tolist() == ["y", "z"]


def test_calculate_matrix_medians():
    X = np.array([[1.0, np.nan, -np.inf, 1e308, -0.0], [3.0, 2.0, np.inf, 1e308, 0.0], [2.0, 4.0, 0.0, 1.0, -0.0]])
    m = ik.calculate_matrix_medians(X, engine=CPU)
    assert m[0] == 2.0 and np.isnan(m[1]) and m[2] == 0.0 and m[3] == 1e308
    assert np.array([m[1]]).view(np.uint64)[0] == 0x7FF00000000007A2
    m = ik.calculate_matrix_medians(X[:2], na_rm=True, engine=CPU)
    assert m.tolist()[0] == 2.0 and m[1] == 2.0 and np.isnan(m[2]) and m[3] == 1e308
    assert np.array([m[2]]).view(np.uint64)[0] == 0x7FF8000000000000   # mean(c(-Inf, Inf))
    assert math.copysign(1.0, m[4]) == 1.0
    rows = ik.calculate_matrix_medians(X, use="row", na_rm=True, engine=CPU)
    np.testing.assert_array_equal(rows, [np.median(r[~np.isnan(r)]) for r in X])
    assert ik.calculate_matrix_medians(X, use="other", engine=CPU)[0] == 2.0
    assert np.isnan(ik.calculate_matrix_medians(np.full((2, 1), np.nan), na_rm=True, engine=CPU)[0])


def test_rank_order_data_numpy_path():
    X = np.array([[1.0, 0.0, 3.0],
                  [0.0, 0.0, 0.0],
                  [5.0, 2.0, np.nan],
                  [2.0, 2.0, 1.0],
                  [-0.0, 7.0, 1.0]])
    r = ik.rank_order_data(X, engine=CPU)
    # rows 1 (all zero) is dropped; ranks with na.last = FALSE over rows 0, 2, 3, 4
    nr = r["n_na_rank"]
    assert nr.index.tolist() == [0, 2, 3, 4]
    assert nr["n_na"].tolist() == [1, 1, 0, 1]
    # rank(na.last = FALSE) of the kept rows 0, 2, 3, 4 (0 and -0 are excluded): column 0 [1, 5, 2, NA] -> 2 4 3 1,
    # column 1 [NA, 2, 2, 7] -> 1 2.5 2.5 4, column 2 [3, NA, 1, 1] -> 4 1 2.5 2.5
    assert nr["median_rank"].tolist() == [2.0, 2.5, 2.5, 2.5]
    assert r["row_order"].tolist() == [2, 3, 4, 0]
    assert r["col_order"].tolist() == [0, 1, 2]
    assert r["ordered"].index.tolist() == r["row_order"].tolist()
    assert "split" not in nr
    both = ik.rank_order_data(X, sample_classes=["b", "a", "b"], engine=CPU)
    assert list(both) == ["a", "b"]
    assert both["a"]["n_na_rank"]["split"].tolist() == ["a"] * len(both["a"]["n_na_rank"])
    none = ik.rank_order_data(np.zeros((3, 2)), engine=CPU)
    assert none is None
