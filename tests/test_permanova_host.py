"""PERMANOVA's host arithmetic without a GPU: api.permanova_statistic, the comparison of labellings, the numpy fallback
api._permanova_numpy and the front end on the CPU oracle, against hand-worked cases, against one-way ANOVA on designed
matrices whose squared dissimilarities are exact, and against the brute-force checker (tests/permanova_checker.py)."""
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

from icikendalltau_amd import api
from tests.oracle_engine import OracleEngine
from tests.permanova_checker import bits, brute_permanova, documented_permutations, na_real, quantise

SCALE = 2 ** 50


def _raw_of_points(x):
    """points on a line -> raw = 1 - |x_i - x_j|: with coordinates at multiples of 1/8 in [0, 2] every raw, every
    d = 1 - raw and every d^2 (a multiple of 1/64, at most 4) is exact"""
    x = np.asarray(x, dtype=np.float64)
    assert np.all(x * 8 == np.round(x * 8)) and x.min() >= 0 and x.max() <= 2
    return 1.0 - np.abs(x[:, None] - x[None, :])


def _stat(raw, cls, n_class):
    """(permanova_statistic of the labelling, the integers) through the numpy fallback"""
    n_pairs, Q, class_q = api._permanova_numpy(raw, cls, n_class, np.zeros((0, len(cls)), dtype=np.int32))
    return api.permanova_statistic(len(cls), Q, class_q[0], np.bincount(cls, minlength=n_class)), n_pairs, Q, class_q


def _anova_f(x, cls):
    """one-way ANOVA of the coordinates, in Fractions: (F or None / inf, SS_between, SS_within)"""
    x = [Fraction(float(v)) for v in x]
    groups = {}
    for v, c in zip(x, cls):
        groups.setdefault(int(c), []).append(v)
    grand = sum(x) / len(x)
    ss_b = sum(len(g) * (sum(g) / len(g) - grand) ** 2 for g in groups.values())
    ss_w = sum(sum((v - sum(g) / len(g)) ** 2 for v in g) for g in groups.values())
    C, S = len(groups), len(x)
    if C < 2 or S <= C or ss_b + ss_w == 0:
        return None, ss_b, ss_w
    if ss_w == 0:
        return math.inf, ss_b, ss_w
    return (ss_b / (C - 1)) / (ss_w / (S - C)), ss_b, ss_w


# ---- hand-worked --------------------------------------------------------------------------------------------------

def test_hand_worked_four_samples():
    # d: (0,1) 1/2, (2,3) 1/4, every pair between the classes 1.  d^2: 1/4, 1/16, and four times 1
    d = np.array([[0, .5, 1, 1], [.5, 0, 1, 1], [1, 1, 0, .25], [1, 1, .25, 0]])
    st, n_pairs, Q, class_q = _stat(1.0 - d, np.array([0, 0, 1, 1]), 2)
    assert list(n_pairs) == [6, 0]
    assert Q == (4 * 64 + 16 + 4) * SCALE // 64 and list(class_q[0]) == [SCALE // 4, SCALE // 16]
    assert st.ss_total == Fraction(69, 64) and st.ss_within == Fraction(1, 8) + Fraction(1, 32)
    assert st.ss_among == Fraction(59, 64) and (st.df_among, st.df_within) == (1, 2)
    assert st.F == Fraction(59, 5) and st.r2 == Fraction(59, 69)
    assert tuple(st) == (st.F, st.r2, st.ss_total, st.ss_within, st.ss_among, 1, 2)


def test_hand_worked_five_samples_three_classes_one_empty():
    # points 0, 1/2 | 1, 3/2, 2 on a line, classes 0 and 2 of three declared: the middle one stays empty
    x = [0, .5, 1, 1.5, 2]
    cls = np.array([0, 0, 2, 2, 2])
    st, _n, Q, class_q = _stat(_raw_of_points(x), cls, 3)
    # sum of d^2 over all pairs = S * sum (x - mean)^2 = 5 * 2.5; within: 2 * (1/8) and 3 * (1/2)
    assert Q == Fraction(25, 2) * SCALE and list(class_q[0]) == [SCALE // 4, 0, 3 * SCALE // 2]
    assert st.ss_total == Fraction(5, 2) and st.ss_within == Fraction(1, 8) + Fraction(1, 2)
    assert (st.df_among, st.df_within) == (1, 3)
    assert st.F == (Fraction(15, 8) / 1) / (Fraction(5, 8) / 3) == 9 and st.r2 == Fraction(3, 4)


def test_hand_worked_six_samples_through_the_comparison():
    x = [0, .125, .25, 1, 1.125, 1.25]
    cls = np.array([0, 0, 0, 1, 1, 1])
    perms = np.array([[1, 1, 1, 0, 0, 0],      # the classes renamed: the same partition, the same F
                      [0, 1, 0, 1, 0, 1],      # a worse split
                      [0, 0, 1, 1, 1, 1],      # other class sizes
                      [0, 0, 0, 0, 0, 0]])     # one class: no F
    n_pairs, Q, class_q = api._permanova_numpy(_raw_of_points(x), cls, 2, perms)
    obs, Fs, n_ge, n_undef = api._permanova_compare(6, Q, class_q, np.vstack([cls[None, :], perms]), 2)
    want = [_anova_f(x, lab)[0] for lab in perms]
    assert obs.F == _anova_f(x, cls)[0] == Fraction(96)       # SS_b = 6 * (1/2)^2 = 3/2, SS_w = 4 / 64, F = (3/2) / ((1/16) / 4)
    assert Fs == want and Fs[0] == obs.F and Fs[3] is None
    assert n_ge == 1 and n_undef == 1


# ---- the designed family: PERMANOVA on Euclidean distances is one-way ANOVA ----------------------------------------------

def _designed(seed, S, sizes):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 17, size=S) / 8.0
    cls = np.repeat(np.arange(len(sizes)), sizes)
    assert len(cls) == S
    rng.shuffle(cls)
    return x, cls.astype(np.int32)


@pytest.mark.parametrize("seed,S,sizes", [(1, 12, (4, 4, 4)), (2, 13, (6, 4, 2, 1)), (3, 9, (1, 8)), (4, 30, (11, 7, 5, 4, 2, 1)),
                                          (5, 6, (3, 3))])
def test_designed_family_equals_anova(seed, S, sizes):
    x, cls = _designed(seed, S, sizes)
    raw = _raw_of_points(x)
    st, n_pairs, Q, class_q = _stat(raw, cls, len(sizes))
    F, ss_b, ss_w = _anova_f(x, cls)
    assert isinstance(F, Fraction) and isinstance(st.F, Fraction)
    assert st.F == F and st.ss_among == ss_b and st.ss_within == ss_w and st.ss_total == ss_b + ss_w
    assert st.r2 == ss_b / (ss_b + ss_w)
    # ... and the checker's integers are the fallback's: every d^2 is exact, so nothing was rounded at all
    ref = brute_permanova(raw, cls, len(sizes), np.zeros((0, S), dtype=np.int32))
    assert ref["q_total"] == Q == sum(round(Fraction(float(a - b)) ** 2 * SCALE) for i, a in enumerate(x) for b in x[i + 1:])
    assert ref["class_q"][0] == list(class_q[0]) and ref["exact"][0][0] == F


def test_designed_family_permutations_equal_anova():
    x, cls = _designed(7, 14, (6, 5, 2, 1))
    perms = documented_permutations(cls, 25, 3)
    res_q = api._permanova_numpy(_raw_of_points(x), cls, 4, perms)
    obs, Fs, n_ge, n_undef = api._permanova_compare(14, res_q[1], res_q[2], np.vstack([cls[None, :], perms]), 4)
    want = [_anova_f(x, lab)[0] for lab in perms]
    assert Fs == want and n_undef == 0
    assert n_ge == sum(1 for f in want if f >= obs.F)


# ---- the quantisation's bound -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,S", [(0, 40), (1, 90)])
def test_quantisation_bound_on_random_raw(seed, S):
    """per pair |q 2^-50 - e| <= 2^-51 (the rounding to an integer), so over M pairs |Q 2^-50 - sum e| <= M 2^-51;
    math.fsum returns the exact sum rounded once: a relative 2^-53 more"""
    rng = np.random.default_rng(seed)
    raw = np.zeros((S, S))
    iu = np.triu_indices(S, k=1)
    raw[iu] = rng.uniform(-1, 1, size=len(iu[0]))
    raw = raw + raw.T
    _n, Q, _c = api._permanova_numpy(raw, np.zeros(S, dtype=np.int32), 1, np.zeros((0, S), dtype=np.int32))
    M = len(iu[0])
    e = [(1.0 - v) * (1.0 - v) for v in raw[iu]]
    total = math.fsum(e)
    err = abs(Fraction(Q, SCALE) - Fraction(total))
    print("M", M, "Q 2^-50", Q / SCALE, "fsum", total, "difference", float(err), "bound", M * 2.0 ** -51 + 2.0 ** -53 * total)
    assert err <= Fraction(M, 2 ** 51) + Fraction(total) / 2 ** 53
    assert Q == sum(quantise(v) for v in raw[iu])


# ---- undefined cases ---------------------------------------------------------------------------------------------------------

def test_one_class_has_no_f():
    x, _cls = _designed(8, 7, (7,))
    st, *_ = _stat(_raw_of_points(x), np.zeros(7, dtype=np.int32), 1)
    assert st.F is None and st.df_among == 0 and st.ss_among == 0 and st.r2 == 0


def test_all_singletons_have_no_f():
    x, _cls = _designed(9, 6, (6,))
    st, _n, _Q, class_q = _stat(_raw_of_points(x), np.arange(6, dtype=np.int32), 6)
    assert st.F is None and st.df_within == 0 and st.ss_within == 0 and not any(class_q[0]) and st.r2 == 1


def test_no_dissimilarity_at_all_has_no_f():
    st, _n, Q, _c = _stat(np.ones((6, 6)), np.array([0, 0, 0, 1, 1, 1]), 2)
    assert Q == 0 and st.ss_total == 0 and st.F is None and st.r2 is None


def test_classes_without_spread_give_inf():
    x = [0.5, 0.5, 0.5, 1.75, 1.75]
    st, *_ = _stat(_raw_of_points(x), np.array([0, 0, 0, 1, 1]), 2)
    assert st.ss_within == 0 and st.ss_among > 0 and st.F == math.inf and st.r2 == 1
    assert _anova_f(x, [0, 0, 0, 1, 1])[0] == math.inf


def test_na_pair_gives_na_everywhere():
    rng = np.random.default_rng(12)
    X = rng.standard_normal((30, 8))
    X[:, 2] = 1.5                                          # a constant column: its seven pairs have no raw
    names = [f"s{i}" for i in range(8)]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = api.ici_kendalltau_permanova(X, list("aabbaabb"), permutations=5, seed=2, colnames=names, engine=OracleEngine())
    assert sum("PERMANOVA needs every pair" in str(x.message) for x in w) == 1
    na = bits(na_real())[0]
    assert res["n_na"] == 7 and res["n_valid"] == 21
    for key in ("statistic", "r2", "pvalue", "ss_total", "ss_within", "ss_among"):
        assert bits(res[key])[0] == na, key
    assert np.all(bits(res["perm_statistic"]) == na) and np.all(bits(res["class_ss"]) == na)
    assert res["n_ge"] == 0 and res["n_undefined"] == 5 and not res["sums"]["class_q"].any()


# ---- the comparison rule ---------------------------------------------------------------------------------------------------

def test_renamed_classes_count_as_ge():
    """a relabelling that only renames the classes is the observed partition: its F is the observed F, exactly, and
    counts -- through SS_W when the sizes sit at the same codes, through the F fraction when they do not"""
    rng = np.random.default_rng(13)
    S = 11
    raw = np.zeros((S, S))
    iu = np.triu_indices(S, k=1)
    raw[iu] = rng.uniform(-1, 1, size=len(iu[0]))
    raw = raw + raw.T
    cls = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2], dtype=np.int32)
    swap01 = np.array([1, 1, 1, 1, 0, 0, 0, 0, 2, 2, 2])         # sizes (4, 4, 3) stay where they are
    rotate = (cls + 1) % 3                                        # sizes become (3, 4, 4)
    perms = np.vstack([swap01, rotate, cls])
    n_pairs, Q, class_q = api._permanova_numpy(raw, cls, 3, perms)
    obs, Fs, n_ge, n_undef = api._permanova_compare(S, Q, class_q, np.vstack([cls[None, :], perms]), 3)
    assert Fs == [obs.F] * 3 and n_ge == 3 and n_undef == 0
    ref = brute_permanova(raw, cls, 3, perms)
    assert ref["n_ge"] == 3 and ref["exact"][1] == Fs


# ---- the fallback and the front end against the checker ------------------------------------------------------------------------

@pytest.mark.parametrize("n_class,kind", [(2, "balanced"), (5, "unequal"), (9, "sparse")])
def test_fallback_equals_the_checker(n_class, kind):
    rng = np.random.default_rng(14)
    S = 23
    raw = np.zeros((S, S))
    iu = np.triu_indices(S, k=1)
    raw[iu] = rng.uniform(-1, 1, size=len(iu[0]))
    raw[0, 1], raw[2, 3], raw[4, 5] = -0.0, 1.0, -1.0
    raw = raw + raw.T
    cls = {"balanced": np.arange(S) % 2, "unequal": np.minimum(np.arange(S) // 5, 4) * (np.arange(S) != 22) + 4 * (np.arange(S) == 22),
           "sparse": (np.arange(S) % 3) * 4}[kind].astype(np.int32)
    perms = np.vstack([documented_permutations(cls, 9, 5), rng.integers(0, n_class, size=(3, S))])   # (other sizes too)
    n_pairs, Q, class_q = api._permanova_numpy(raw, cls, n_class, perms)
    ref = brute_permanova(raw, cls, n_class, perms)
    assert np.array_equal(n_pairs, ref["n_pairs"]) and Q == ref["q_total"]
    assert [list(row) for row in class_q] == ref["class_q"]
    obs, Fs, n_ge, n_undef = api._permanova_compare(S, Q, class_q, np.vstack([cls[None, :], perms]), n_class)
    assert tuple(obs) == ref["exact"][0] and Fs == ref["exact"][1]
    assert (n_ge, n_undef) == (ref["n_ge"], ref["n_undefined"])


@pytest.mark.parametrize("strata", [None, "halves"])
def test_front_end_on_the_oracle_equals_the_checker(strata):
    rng = np.random.default_rng(15)
    S, n = 14, 40
    X = rng.standard_normal((n, S))
    X[rng.random((n, S)) < 0.1] = np.nan
    names = [f"s{i}" for i in range(S)]
    codes = np.array([0, 1, 2, 0, 1, 2, 0, 1, 0, 1, 0, 0, 3, 1], dtype=np.int32)
    labels = [f"c{k}" for k in codes]
    st = None if strata is None else ["l"] * 6 + ["r"] * 8
    eng = OracleEngine()
    got = api.ici_kendalltau_permanova(X, labels, permutations=19, seed=4, strata=st, colnames=names, engine=eng)
    raw = np.asarray(api.ici_kendalltau(X, colnames=names, engine=eng)["raw"])
    ref = brute_permanova(raw, codes, 4, documented_permutations(codes, 19, 4, st))
    assert got["n_valid"] == ref["n_pairs"][0] and got["n_na"] == 0
    assert got["sums"]["q_total"] == ref["q_total"] and [list(r) for r in got["sums"]["class_q"]] == ref["class_q"]
    assert (got["n_ge"], got["n_undefined"]) == (ref["n_ge"], ref["n_undefined"])
    assert (got["df_among"], got["df_within"]) == (ref["df_among"], ref["df_within"]) == (3, 10)
    assert np.array_equal(got["class_size"], ref["class_size"])
    for key in ("statistic", "r2", "pvalue", "ss_total", "ss_within", "ss_among", "perm_statistic", "class_ss"):
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
    # the same (seed, strata) give ANOSIM the same labellings
    assert np.array_equal(api.anosim_permutations(codes, 19, 4, st), documented_permutations(codes, 19, 4, st))
