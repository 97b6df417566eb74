"""The host side of the Mantel test without a GPU: the brute-force checker on cases worked by
hand and on every permutation of four and five samples, the statistic against independent references (scipy's
spearmanr, numpy's corrcoef, a 120-digit decimal evaluation), the permutation contract, the front end on an engine
without a mantel method (tests/oracle_engine.py: the S x S raw of the CPU oracle, then api._mantel_numpy), and the
plain C++ header csrc/icikt_mantel.h compiled alone (tests/mantel_print.cpp, with the address and undefined-behaviour
sanitizers where they link)."""
import decimal
import itertools
import json
import math
import os
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

from icikendalltau_amd import api
from tests.mantel_checker import (bits, brute_mantel, condensed, documented_permutations, na_real, quantise_x, quantise_y,
                                  rank2, rank2_loops, statistic)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "mantel_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")


def _raw_of(S, d):
    """the S x S raw matrix whose dissimilarities 1 - raw are d, in combn order (diagonal 1)"""
    raw = np.eye(S)
    iu, ju = np.triu_indices(S, k=1)
    raw[iu, ju] = raw[ju, iu] = 1.0 - np.asarray(d, dtype=np.float64)
    return raw


def _random_raw(S, seed):
    rng = np.random.default_rng(seed)
    return _raw_of(S, rng.uniform(0.0, 2.0, size=S * (S - 1) // 2))


def _all_perms(S):
    return np.array(list(itertools.permutations(range(S))), dtype=np.int32)


def _is_na(v):
    return bits(v)[0] == bits(na_real())[0]


# ---- the checker on cases worked by hand -------------------------------------------------------------------------------

def test_three_samples_by_hand():
    raw = _raw_of(3, [0.5, 0.75, 1.0])                 # pairs (0,1), (0,2), (1,2)
    other = [3.0, 1.0, 2.0]
    swap01 = [[1, 0, 2]]                               # y of pair (0,1) -> y10 = 3, (0,2) -> y12 = 2, (1,2) -> y02 = 1
    for loops in (True, False):
        sp = brute_mantel(raw, other, "spearman", swap01, loops=loops)
        assert list(sp["xv"]) == [2, 4, 6] and list(sp["yv"]) == [6, 2, 4]
        assert sp["T"] == [2 * 6 + 4 * 2 + 6 * 4, 2 * 6 + 4 * 4 + 6 * 2] and sp["moments"] == (12, 56, 12, 56)
        assert sp["statistic"] == -0.5 and sp["perm_statistic"][0] == -1.0       # (3 * 44 - 144) / 24, (3 * 40 - 144) / 24
        assert (sp["n_ge"], sp["n_le"]) == (0, 1) and sp["pvalue"] == 0.5
        pe = brute_mantel(raw, other, "pearson", swap01, loops=loops)
        assert list(pe["xv"]) == [2 ** 29, 3 * 2 ** 28, 2 ** 30]
        assert list(pe["yv"]) == [2 ** 30, 0, 2 ** 29]                           # lo = 1, span = 2 = 0.5 * 2^2: (y - 1) 2^29
        assert pe["T"] == [2 ** 59 + 2 ** 59, 2 ** 59 + 3 * 2 ** 57 + 0]
        assert pe["statistic"] == -0.5 and pe["perm_statistic"][0] == -1.0
        assert list(pe["n_pairs"]) == [3, 0]


def test_loops_and_pieces_agree():
    for S, seed in ((6, 1), (9, 2)):
        raw = _random_raw(S, seed)
        raw[0, 1] = raw[1, 0] = raw[2, 3] = raw[3, 2] = -0.0 if S == 6 else 0.25      # ties, and -0 beside +0
        raw[0, 2] = raw[2, 0] = 0.0 if S == 6 else 0.25
        other = np.random.default_rng(seed + 10).integers(0, 4, size=S * (S - 1) // 2).astype(float)
        perms = documented_permutations(S, 7, seed)
        for method in ("pearson", "spearman"):
            a, b = brute_mantel(raw, other, method, perms, loops=True), brute_mantel(raw, other, method, perms)
            assert a["T"] == b["T"] and a["moments"] == b["moments"] and (a["n_ge"], a["n_le"]) == (b["n_ge"], b["n_le"])
            assert list(a["xv"]) == list(b["xv"]) and list(a["yv"]) == list(b["yv"])
            assert np.array_equal(bits(a["perm_statistic"]), bits(b["perm_statistic"]))
    v = [0.5, -0.0, 0.0, 0.5, 2.0]
    assert rank2_loops(v) == list(rank2(v)) == [7, 3, 3, 7, 10]


def test_four_samples_every_permutation_of_a_design_matrix():
    """d of the pairs 01, 02, 03, 12, 13, 23 and the 0/1 design {0, 1} | {2, 3}: a permutation only chooses which of
    the three pairings of four samples is `within`; each is chosen by 8 of the 24 permutations.  Between-group sums of
    the doubled ranks (2, 6, 10, 12, 8, 4; total 42): 42 - (2 + 4) = 36 for 01|23 (the identity's), 42 - (6 + 8) = 28
    for 02|13, 42 - (10 + 12) = 20 for 03|12."""
    d = [0.125, 0.375, 0.625, 0.75, 0.5, 0.25]
    raw = _raw_of(4, d)
    design = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0]], dtype=float)
    perms = _all_perms(4)
    sp = brute_mantel(raw, design, "spearman", perms, loops=True)
    assert list(sp["xv"]) == [2, 6, 10, 12, 8, 4] and list(sp["yv"]) == [3, 9, 9, 9, 9, 3]   # y: two 0s (ranks 1.5), four 1s (4.5)
    # T = 3 * within + 9 * between = 3 * 42 + 6 * between
    assert sorted(set(sp["T"])) == [126 + 6 * 20, 126 + 6 * 28, 126 + 6 * 36] and sp["T"][0] == 126 + 6 * 36
    assert [sp["T"][1:].count(t) for t in sorted(set(sp["T"]))] == [8, 8, 8]
    assert (sp["n_ge"], sp["n_le"]) == (8, 24) and sp["pvalue"] == 9 / 25
    pe = brute_mantel(raw, design, "pearson", perms, loops=True)
    # xv = d 2^30, yv = y 2^30 (lo = 0, span = 1 = 0.5 * 2^1): T = 2^60 * (the between-group sum of d)
    assert sorted(set(pe["T"])) == [5 << 58, 7 << 58, 9 << 58] and pe["T"][0] == 9 << 58
    assert (pe["n_ge"], pe["n_le"]) == (8, 24)
    # equal T everywhere: d whose three pairings all sum to the same
    flat = brute_mantel(_raw_of(4, [0.125, 0.25, 0.375, 0.5, 0.625, 0.75]), design, "pearson", perms, loops=True)
    assert len(set(flat["T"])) == 1 and (flat["n_ge"], flat["n_le"]) == (24, 24) and flat["pvalue"] == 1.0
    assert flat["statistic"] == flat["perm_statistic"][5]


def test_five_samples_every_permutation():
    """run order |t_i - t_j| against designed dissimilarities: the counts from exact fractions of the doubles"""
    d = [0.125, 0.5, 0.75, 1.0, 0.25, 0.625, 0.875, 0.375, 0.5, 0.125]       # with ties
    raw = _raw_of(5, d)
    t = np.arange(5.0)
    other = np.abs(t[:, None] - t[None, :])
    perms = _all_perms(5)
    pairs = list(itertools.combinations(range(5), 2))
    exact = [sum(Fraction(dd) * Fraction(other[p[i], p[j]]) for (i, j), dd in zip(pairs, d)) for p in perms.tolist()]
    want_ge, want_le = sum(e >= exact[0] for e in exact), sum(e <= exact[0] for e in exact)
    assert (want_ge, want_le) == (2, 120)               # the identity and its reversal (the same |t_i - t_j|) give the largest sum
    pe = brute_mantel(raw, other, "pearson", perms, loops=True)
    # dyadic inputs: the integers are the values scaled, xv = d 2^30 and yv = (y - 1) 2^29 (lo = 1, span = 3 = 0.75 * 2^2)
    assert pe["T"][1:] == [int((e - sum(Fraction(dd) for dd in d)) * 2 ** 59) for e in exact]
    assert (pe["n_ge"], pe["n_le"]) == (want_ge, want_le) and pe["pvalue"] == 3 / 121
    for method in ("pearson", "spearman"):
        a = brute_mantel(raw, other, method, perms, loops=True)
        b = api._mantel_numpy(raw, condensed(other, 5), method, perms)
        assert list(b[1]) == a["T"] and b[2] == a["moments"] and (b[3], b[4]) == (a["n_ge"], a["n_le"])


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_other_equal_to_the_dissimilarity_gives_one(method):
    S = 7
    rng = np.random.default_rng(3)
    d = rng.integers(0, 17, size=21) / 8.0                  # dyadic, with ties: both quantisations are exact
    raw = _raw_of(S, d)
    perms = documented_permutations(S, 40, 5)
    perms[3] = np.arange(S)                                 # the identity reproduces T
    ref = brute_mantel(raw, 1.0 - raw, method, perms)
    assert ref["statistic"] == 1.0 and ref["perm_statistic"][3] == 1.0
    assert ref["n_ge"] == sum(1 for t in ref["T"][1:] if t == ref["T"][0]) >= 1 and ref["n_le"] == 40
    P, (sx, sxx, sy, syy) = 21, ref["moments"]
    assert (P * ref["T"][0] - sx * sy) ** 2 == (P * sxx - sx * sx) * (P * syy - sy * sy)       # exactly 1
    down = brute_mantel(raw, 3.0 * raw + 2.0, method, perms)                                    # = 5 - 3 (1 - raw)
    assert down["statistic"] == -1.0 and down["n_le"] == down["T"][1:].count(down["T"][0]) >= 1 and down["n_ge"] == 40
    assert api.mantel_statistic(P, ref["T"][0], *ref["moments"]) == 1.0
    assert api.mantel_statistic(P, down["T"][0], *down["moments"]) == -1.0


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_constant_other_and_na_pairs_give_na(method):
    S = 6
    raw = _random_raw(S, 9)
    perms = documented_permutations(S, 5, 1)
    const = brute_mantel(raw, np.full(15, 2.5), method, perms)
    assert _is_na(const["statistic"]) and _is_na(const["pvalue"]) and all(_is_na(v) for v in const["perm_statistic"])
    assert list(const["n_pairs"]) == [15, 0] and (const["n_ge"], const["n_le"]) == (5, 5)       # every T is equal
    assert api.mantel_statistic(15, const["T"][0], *const["moments"]) is None
    raw[1, 4] = raw[4, 1] = np.nan
    other = np.arange(15.0)
    na = brute_mantel(raw, other, method, perms)
    assert list(na["n_pairs"]) == [14, 1] and na["T"] == [0] * 6 and na["moments"] == (0, 0, 0, 0)
    assert (na["n_ge"], na["n_le"]) == (0, 0) and _is_na(na["statistic"]) and _is_na(na["pvalue"])
    got = api._mantel_numpy(raw, other, method, perms)
    assert list(got[0]) == [14, 1] and list(got[1]) == [0] * 6 and got[2] == (0, 0, 0, 0) and got[3:] == (0, 0)


# ---- accuracy against independent references --------------------------------------------------------------------------

def _pairs_of(S, seed, ties):
    rng = np.random.default_rng(seed)
    P = S * (S - 1) // 2
    d = rng.uniform(0.0, 2.0, size=P)
    y = 0.3 * d + rng.standard_normal(P) * (2.0 ** rng.integers(-8, 9))
    if ties:
        d, y = np.round(d * 8) / 8, np.round(y * 2) / 2
    return _raw_of(S, d), d, y


@pytest.mark.parametrize("S", [5, 12, 40, 100, 300])
@pytest.mark.parametrize("ties", [False, True])
def test_spearman_against_scipy(S, ties):
    stats = pytest.importorskip("scipy.stats")
    raw, d, y = _pairs_of(S, 100 + S, ties)
    ref = brute_mantel(raw, y, "spearman", np.zeros((0, S), dtype=np.int32))
    want = float(stats.spearmanr(1.0 - raw[np.triu_indices(S, k=1)], y)[0])
    print("S", S, "ties", ties, "r", ref["statistic"], "scipy", want, "difference", abs(ref["statistic"] - want))
    assert abs(ref["statistic"] - want) <= 1e-12
    assert api.mantel_statistic(S * (S - 1) // 2, ref["T"][0], *ref["moments"]) == ref["statistic"]


@pytest.mark.parametrize("S", [5, 12, 40, 100, 300])
@pytest.mark.parametrize("ties", [False, True])
def test_pearson_against_numpy_within_the_quantisation_bound(S, ties):
    """each value moves by at most 2^-31 of its scale (x: of 1; y: of 2^e >= span): to first order r moves by at most
    2^-30 (1 / sd(x) + span / sd(y)); the factor 2 is margin for second order and for numpy's own rounding"""
    raw, _d, y = _pairs_of(S, 200 + S, ties)
    x = 1.0 - raw[np.triu_indices(S, k=1)]
    ref = brute_mantel(raw, y, "pearson", np.zeros((0, S), dtype=np.int32))
    want = float(np.corrcoef(x, y)[0, 1])
    bound = 2.0 ** -29 * (1.0 / np.std(x, ddof=1) + (y.max() - y.min()) / np.std(y, ddof=1))
    print("S", S, "ties", ties, "r", ref["statistic"], "numpy", want, "difference", abs(ref["statistic"] - want), "bound", bound)
    assert abs(ref["statistic"] - want) <= bound
    assert api.mantel_statistic(S * (S - 1) // 2, ref["T"][0], *ref["moments"]) == ref["statistic"]


def test_statistic_against_a_120_digit_evaluation():
    rng = np.random.default_rng(77)
    cases = [(3, 44, 12, 56, 12, 56), (3, 40, 12, 56, 12, 56)]
    for _ in range(300):
        P = int(rng.integers(2, 2000))
        x = rng.integers(0, 2 ** 31 + 1, size=P).astype(object)
        y = rng.integers(0, 2 ** 31 + 1, size=P).astype(object) if rng.random() < 0.5 else x * int(rng.integers(1, 4)) + rng.integers(0, 3, size=P).astype(object)
        cases.append((P, int(np.sum(x * y)), int(np.sum(x)), int(np.sum(x * x)), int(np.sum(y)), int(np.sum(y * y))))
    for P, T, sx, sxx, sy, syy in cases:
        with decimal.localcontext() as ctx:
            ctx.prec = 120
            want = float(decimal.Decimal(P * T - sx * sy) / (decimal.Decimal(P * sxx - sx * sx) * decimal.Decimal(P * syy - sy * sy)).sqrt())
        got = api.mantel_statistic(P, T, sx, sxx, sy, syy)
        assert got == want and got == statistic(P, T, sx, sxx, sy, syy), (P, T, got, want)
        assert -1.0 <= got <= 1.0
    assert api.mantel_statistic(5, 10, 5, 5, 7, 20) is None and api.mantel_statistic(0, 0, 0, 0, 0, 0) is None
    assert api._sqrt_fraction(1, 4) == 0.5 and api._sqrt_fraction(2, 1) == math.sqrt(2.0) and api._sqrt_fraction(0, 3) == 0.0
    assert api._sqrt_fraction(10 ** 400, 1) == 1e200 and api._sqrt_fraction(1, 10 ** 400) == 1e-200


# ---- the permutation contract ------------------------------------------------------------------------------------------

def test_permuting_codes_is_indexing_by_a_permutation():
    """what lets one seed serve ANOSIM, PERMANOVA, PERMDISP and Mantel: numpy shuffles positions, whatever they hold"""
    for S in range(2, 301):
        codes = np.random.default_rng(S).integers(0, 5, size=S).astype(np.int32)
        a = np.random.default_rng(S + 1000).permutation(codes)
        b = codes[np.random.default_rng(S + 1000).permutation(S)]
        assert np.array_equal(a, b), S


@pytest.mark.parametrize("strata", [None, "three"])
def test_mantel_permutations_contract(strata):
    S = 23
    st = None if strata is None else ["a"] * 7 + ["b"] * 10 + ["c"] * 6
    perms = api.mantel_permutations(S, 12, seed=4, strata=st)
    assert perms.dtype == np.int32 and perms.shape == (12, S)
    assert np.array_equal(perms, documented_permutations(S, 12, 4, st))
    assert all(sorted(row.tolist()) == list(range(S)) for row in perms)
    codes = np.random.default_rng(8).integers(0, 4, size=S).astype(np.int32)
    assert np.array_equal(codes[perms], api.anosim_permutations(codes, 12, seed=4, strata=st))
    if st is not None:
        assert all(st[s] == st[int(v)] for row in perms for s, v in enumerate(row))
    given = perms[:3].astype(np.int64)
    assert np.array_equal(api.mantel_permutations(S, given), perms[:3])
    with pytest.raises(ValueError):
        api.mantel_permutations(S, -1)


# ---- the front end on an engine without a mantel method ----------------------------------------------------------------

def _front_data():
    S, n = 12, 30
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.standard_normal((n, S)) + 1.5 * rng.standard_normal((n, 1)))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X, [f"s{i}" for i in range(S)], S


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_front_end_on_an_engine_without_mantel(method):
    from tests.oracle_engine import OracleEngine
    X, names, S = _front_data()
    t = np.random.default_rng(2).uniform(0, 10, size=S)
    other = np.abs(t[:, None] - t[None, :])
    eng = OracleEngine()
    full = api.ici_kendalltau(X, colnames=names, engine=eng)
    got = api.ici_kendalltau_mantel(X, other, method=method, permutations=20, seed=7, colnames=names, engine=eng)
    assert list(got) == ["statistic", "pvalue", "n_permutations", "n_ge", "n_le", "n_valid", "n_na", "perm_statistic", "method",
                         "sums", "sample_id", "max_taumax", "run_time"]
    ref = brute_mantel(np.asarray(full["raw"]), other, method, documented_permutations(S, 20, 7))
    assert got["n_permutations"] == 20 and got["method"] == method and got["sample_id"] == names
    assert (got["n_valid"], got["n_na"]) == (66, 0) and (got["n_ge"], got["n_le"]) == (ref["n_ge"], ref["n_le"])
    assert list(got["sums"]["T"]) == ref["T"]
    assert (got["sums"]["sx"], got["sums"]["sxx"], got["sums"]["sy"], got["sums"]["syy"]) == ref["moments"]
    for key in ("statistic", "pvalue", "perm_statistic"):
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
    # the condensed form, an explicit array of permutations, and no perm_statistic
    short = api.ici_kendalltau_mantel(X, condensed(other, S), method=method, permutations=documented_permutations(S, 20, 7),
                                      colnames=names, engine=eng, return_perms=False)
    assert "perm_statistic" not in short and list(short) == [k for k in got if k != "perm_statistic"]
    assert bits(short["statistic"])[0] == bits(got["statistic"])[0] and short["n_ge"] == got["n_ge"]
    assert list(short["sums"]["T"]) == ref["T"]
    st = ["l"] * 5 + ["r"] * 7
    strat = api.ici_kendalltau_mantel(X, other, method=method, permutations=9, seed=3, strata=st, colnames=names, engine=eng)
    ref_s = brute_mantel(np.asarray(full["raw"]), other, method, documented_permutations(S, 9, 3, st))
    assert list(strat["sums"]["T"]) == ref_s["T"] and np.array_equal(bits(strat["perm_statistic"]), bits(ref_s["perm_statistic"]))


def test_front_end_na_pairs_warn_and_give_na():
    from tests.oracle_engine import OracleEngine
    X, names, S = _front_data()
    X[:, 11] = 3.0                                               # constant: NA pairs
    other = np.arange(66.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = api.ici_kendalltau_mantel(X, other, permutations=6, seed=1, colnames=names, engine=OracleEngine())
    assert any("`ici_kendalltau_medians` returns `n_valid`" in str(x.message) for x in w)
    assert (got["n_valid"], got["n_na"], got["n_ge"], got["n_le"]) == (55, 11, 0, 0)
    assert _is_na(got["statistic"]) and _is_na(got["pvalue"]) and all(_is_na(v) for v in got["perm_statistic"])
    assert list(got["sums"]["T"]) == [0] * 7


def test_front_end_refusals():
    from tests.oracle_engine import OracleEngine
    X, names, S = _front_data()
    eng = OracleEngine()
    good = np.abs(np.arange(S)[:, None] - np.arange(S)[None, :]).astype(float)

    def call(other, **kw):
        return api.ici_kendalltau_mantel(X, other, colnames=names, engine=eng, **{"permutations": 3, "seed": 0, **kw})

    with pytest.raises(ValueError, match=r"`other` must be an S x S matrix or a condensed vector of length S \(S - 1\) / 2 \(S = 12: 66\), not of shape \(65,\)"):
        call(np.zeros(65))
    with pytest.raises(ValueError, match=r"not of shape \(12, 11\)"):
        call(good[:, :11])
    with pytest.raises(ValueError, match=r"not of shape \(2, 3, 4\)"):
        call(np.zeros((2, 3, 4)))
    skew = good.copy()
    skew[7, 2] += 2.0 ** -40
    with pytest.raises(ValueError, match=r"`other` must be exactly symmetric: other\[2, 7\] = 5\.0 but other\[7, 2\] = 5\.00000"):
        call(skew)
    for bad, text in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
        hole = good.copy()
        hole[3, 9] = hole[9, 3] = bad
        with pytest.raises(ValueError, match=rf"`other` must be finite: the value of pair \(3, 9\) is {text}"):
            call(hole)
        vec = condensed(good, S)
        vec[0] = bad
        with pytest.raises(ValueError, match=rf"the value of pair \(0, 1\) is {text}"):
            call(vec)
    wide = condensed(good, S)
    wide[0], wide[1] = -1.5e308, 1.5e308
    with pytest.raises(ValueError, match="the span of `other`"):
        call(wide)
    call(wide, method="spearman")                       # ranks need no span
    with pytest.raises(ValueError, match="`other` must be numeric"):
        call(np.array([["a"] * S] * S, dtype=object))
    with pytest.raises(ValueError, match='`method` must be "pearson" or "spearman"'):
        call(good, method="kendall")
    twice = np.tile(np.arange(S, dtype=np.int32), (2, 1))
    twice[1, 4] = 5
    with pytest.raises(ValueError, match=r"every row of `permutations` must be a permutation of 0 \.\. S - 1"):
        call(good, permutations=twice)
    with pytest.raises(ValueError, match="`permutations` must be a count or an integer array"):
        call(good, permutations=np.zeros((2, S - 1), dtype=np.int32))
    with pytest.raises(ValueError, match="`strata` must give one stratum per column"):
        call(good, strata=[0, 1])
    diag = good.copy()
    np.fill_diagonal(diag, np.nan)                      # the diagonal is ignored
    assert call(diag)["sums"]["T"][0] == call(good)["sums"]["T"][0]


def test_entries_are_declared_exported_and_built():
    import re
    from icikendalltau_amd import _lib
    import icikendalltau_amd
    with open(os.path.join(ROOT, "include", "icikt.h")) as f:
        header = f.read()
    for nm in ("icikt_mantel_f64", "icikt_mantel_in", "icikt_mantel_csc"):
        assert nm in _lib.EXPORTS and re.search(r"\bint " + nm + r"\(", header), nm
    for f in ("icikt_mantel.hip", "icikt_capi_mantel.cpp"):
        assert os.path.join(CSRC, f) in _lib.SOURCES
    assert os.path.join(CSRC, "icikt_mantel.h") in _lib.HEADERS
    assert all(os.path.exists(p) for p in _lib.SOURCES + _lib.HEADERS)
    assert _lib.MANTEL == {"pearson": 0, "spearman": 1} and _lib.MANTEL_MAX_PERM == 1000000
    assert "#define ICIKT_MANTEL_MAX_PERM 1000000" in header and "#define ICIKT_MANTEL_SPEARMAN 1" in header
    for name in ("ici_kendalltau_mantel", "mantel_permutations", "mantel_statistic"):
        assert getattr(icikendalltau_amd, name) is getattr(api, name)
    assert hasattr(_lib.Context, "mantel") and hasattr(api.HipEngine, "mantel")


# ---- the header alone --------------------------------------------------------------------------------------------------

def _words(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


X_NAMED = np.array([1.0, -1.0, 0.0, -0.0, 1.0 - 2.0 ** -53, np.nan, 1.0 - 2.0 ** -31, 1.0 - 3 * 2.0 ** -31, 1.0 - 5 * 2.0 ** -31])
X_RANDOM = np.random.default_rng(2051).uniform(-1.0, 1.0, size=6000)
Y_SETS = {
    "plain": np.random.default_rng(1).standard_normal(6000 + len(X_NAMED)),
    "wide": np.ldexp(np.random.default_rng(2).uniform(0.5, 1.0, size=500), np.random.default_rng(3).integers(-20, 21, size=500)),
    "negative": -np.abs(np.random.default_rng(4).standard_normal(500)) - 3.0,
    "design": np.random.default_rng(5).integers(0, 2, size=500).astype(float),
    "halves": np.array([0.0, 2.0 ** 31, 1.0, 3.0, 5.0, 7.0, 2.0 ** 31 - 1.0]),    # span = 2^31 = 0.5 * 2^32: yv = rint(y / 2)
    "constant": np.full(9, 7.25),
    "tiny": np.array([1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -51]),
}
COMPARES = [(0, 0, 0, 0), (5, 0, 4, 0), (0, 1, 2 ** 32, 0), (2 ** 32 + 1, 0, 0, 1), (2 ** 62, 2 ** 62, 2 ** 62 + 1, 2 ** 62),
            (2 ** 63 - 1, 1, 2 ** 63 - 1 - 2 ** 32, 2), (7, 2 ** 62, 8, 2 ** 62 - 1)]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    prog = str(tmp_path_factory.mktemp("mantel") / "mantel_print")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", prog]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:   # (no sanitizer runtime here)
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return prog


def _run(prog, xs=(), ys=(), cmps=()):
    text = "".join(f"x {int(w)}\n" for w in _words(np.asarray(xs, dtype=np.float64)))
    text += "".join(f"y {int(w)}\n" for w in _words(np.asarray(ys, dtype=np.float64)))
    text += "".join("c %d %d %d %d\n" % c for c in cmps)
    r = subprocess.run([prog], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def _limb_sums(values):
    lo = sum(int(v) & 0xFFFFFFFF for v in values)
    hi = sum(int(v) >> 32 for v in values)
    return lo, hi


def test_header_x_quantisation_and_limb_sums(prog):
    xs = np.concatenate([X_NAMED, X_RANDOM])
    out = _run(prog, xs, Y_SETS["plain"], COMPARES)
    assert (out["x_frac_bits"], out["y_bits"], out["v_max"], out["methods"]) == (30, 31, 2 ** 31, [0, 1])
    assert out["limbs"] == [0x76543210, 0xFEDCBA98]
    # 1, -1, 0, -0, the double below 1, NaN; then halves: 0.5 rounds to 0, 1.5 to 2, 2.5 to 2
    assert out["xv"][:9] == [0, 2 ** 31, 2 ** 30, 2 ** 30, 0, None, 0, 2, 2]
    assert out["xv_key"][:9] == out["xv"][:9]
    want = api._mantel_quantise_x(X_RANDOM)
    assert out["xv"][9:] == [int(v) for v in want] == quantise_x(X_RANDOM) and out["xv_key"][9:] == out["xv"][9:]
    for k in range(0, len(X_RANDOM), 11):
        assert out["xv"][9 + k] == round(Fraction(1.0 - X_RANDOM[k]) * 2 ** 30)
    assert 0 <= want.min() and want.max() <= 2 ** 31 and len(set(want.tolist())) > 5900
    yv = api._mantel_quantise_y(Y_SETS["plain"])
    assert out["yv"] == [int(v) for v in yv]
    xk = [0 if v is None else v for v in out["xv_key"]]
    prods = [a * int(b) for a, b in zip(xk, yv)]
    assert tuple(out["t"]) == _limb_sums(prods) and (out["t"][1] << 32) + out["t"][0] == sum(prods)
    assert out["t"][0] > 2 ** 32                                        # the low limb alone is past a word
    assert tuple(out["mx"]) == _limb_sums(xk) + _limb_sums([v * v for v in xk])
    assert tuple(out["my"]) == _limb_sums(yv.tolist()) + _limb_sums([int(v) ** 2 for v in yv])
    big = lambda lo, hi: (hi << 32) + lo
    assert out["cmp"] == [(big(a, b) > big(c, d)) - (big(a, b) < big(c, d)) for a, b, c, d in COMPARES]
    assert set(out["cmp"]) == {-1, 0, 1}


@pytest.mark.parametrize("name", sorted(Y_SETS))
def test_header_y_quantisation(prog, name):
    y = Y_SETS[name]
    out = _run(prog, ys=y)
    lo, hi = float(y.min()), float(y.max())
    assert out["lo"] == int(_words(lo)[0]) and out["hi"] == int(_words(hi)[0]) and out["span"] == int(_words(hi - lo)[0])
    assert out["e"] == math.frexp(hi - lo)[1]
    assert out["yv"] == [int(v) for v in api._mantel_quantise_y(y)] == quantise_y(y)
    assert min(out["yv"]) == 0 and max(out["yv"]) <= 2 ** 31
    for k in range(0, len(y), 7):                                       # the exact rational, rounded half to even
        assert out["yv"][k] == round(Fraction(float(y[k]) - lo) * Fraction(2) ** (31 - out["e"]))
    if name == "halves":
        assert out["e"] == 32 and out["yv"] == [0, 2 ** 30, 0, 2, 2, 4, 2 ** 30]      # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4: to even
    if name == "constant":
        assert out["e"] == 0 and set(out["yv"]) == {0}
    if name == "design":
        assert set(out["yv"]) == {0, 2 ** 30}
    if name == "tiny":
        assert out["e"] == -50 and out["yv"] == [0, 2 ** 29, 2 ** 30]
    if name != "constant":
        assert max(out["yv"]) >= 2 ** 30                               # span = m 2^e with m >= 0.5: the top bit's range is used
