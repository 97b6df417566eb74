"""The ANOSIM checker (tests/anosim_checker.py) pinned on closed forms, and the front end's host-side parts that need no
device: the permutation contract, the exact statistic, and the fallback for engines without an anosim method."""
import itertools
import warnings
from fractions import Fraction

import numpy as np
import pytest

from icikendalltau_amd import api
from tests.anosim_checker import (bits, brute_anosim, documented_permutations, doubled_ranks, na_real, statistic,
                                  triangle_values)


def _sym(S, cells):
    raw = np.full((S, S), np.nan)
    np.fill_diagonal(raw, 1.0)
    for (i, j), v in cells.items():
        raw[i, j] = raw[j, i] = v
    return raw


# S = 4, classes (a, a, b, b).  Ranks in descending raw: (0,1) 1, (2,3) 2, (0,2) 3, (0,3) 4, (1,2) 5, (1,3) 6.
_FOUR = _sym(4, {(0, 1): 0.9, (2, 3): 0.8, (0, 2): 0.4, (0, 3): 0.3, (1, 2): 0.2, (1, 3): 0.1})


def test_designed_four_samples_all_relabellings():
    """Observed: within ranks 1, 2 (mean 1.5), between 3 .. 6 (mean 4.5), M / 2 = 3: R = (4.5 - 1.5) / 3 = 1.
    The 24 permutations of (0, 0, 1, 1) give each of the partitions {01|23}, {02|13}, {03|12} 8 times.  {02|13}: within
    ranks 3, 6 (mean 4.5), between 1, 2, 4, 5 (mean 3): R = -1/2.  {03|12}: within 4, 5, the same means: R = -1/2.  So
    8 of the 24 reach R = 1: n_ge = 8, p = (1 + 8) / (1 + 24) = 9 / 25."""
    cls = np.array([0, 0, 1, 1])
    perms = np.array(list(itertools.permutations(cls)))
    assert perms.shape == (24, 4)
    res = brute_anosim(_FOUR, cls, 2, perms)
    assert list(res["r2"]) == [2, 6, 8, 10, 12, 4]            # combn order: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    assert list(res["n_pairs"]) == [6, 0]
    assert res["w2"][0] == 6 and res["nw"][0] == 2
    assert res["exact"][0] == 1 and res["statistic"] == 1.0
    assert sorted(set(res["exact"][1])) == [Fraction(-1, 2), Fraction(1)]
    assert res["n_ge"] == 8 and res["n_undefined"] == 0
    assert res["pvalue"] == 9 / 25 == float(Fraction(9, 25))
    assert list(res["class_w2"]) == [2, 4] and list(res["class_nw"]) == [1, 1]
    assert list(res["class_mean_rank"]) == [1.0, 2.0]
    assert res["within_mean_rank"] == 1.5 and res["between_mean_rank"] == 4.5
    assert np.array_equal(res["perm_statistic"] == 1.0, [tuple(p) in ((0, 0, 1, 1), (1, 1, 0, 0)) for p in perms])


def test_fully_tied_raw_gives_zero():
    raw = _sym(5, {p: 0.25 for p in itertools.combinations(range(5), 2)})
    res = brute_anosim(raw, [0, 0, 1, 1, 1], 2, np.array([[1, 0, 1, 0, 1]]))
    assert set(res["r2"]) == {11} and res["n_pairs"][0] == 10    # every rank is (M + 1) / 2, doubled M + 1
    assert res["exact"][0] == 0 and res["statistic"] == 0.0
    assert res["n_ge"] == 1 and res["pvalue"] == 1.0


def test_negative_zero_ties_with_zero():
    raw = _sym(3, {(0, 1): -0.0, (0, 2): 0.0, (1, 2): -0.5})
    _i, _j, v, M, n_na = triangle_values(raw)
    assert (M, n_na) == (3, 0) and list(doubled_ranks(v)) == [3, 3, 6]


def test_one_class_and_singletons_are_undefined():
    one = brute_anosim(_FOUR, [0, 0, 0, 0], 1, np.zeros((2, 4), dtype=int))
    assert one["exact"][0] is None and one["nw"][0] == 6
    assert bits(one["statistic"])[0] == bits(na_real())[0] == 0x7FF00000000007A2
    assert bits(one["pvalue"])[0] == 0x7FF00000000007A2
    assert one["n_ge"] == 0 and one["n_undefined"] == 2
    single = brute_anosim(_FOUR, [0, 1, 2, 3], 4, np.array([[3, 2, 1, 0]]))
    assert single["exact"][0] is None and single["nw"][0] == 0 and single["n_undefined"] == 1
    assert all(bits(x)[0] == 0x7FF00000000007A2 for x in single["class_mean_rank"])
    assert bits(single["within_mean_rank"])[0] == 0x7FF00000000007A2 and single["between_mean_rank"] == 3.5
    assert statistic(0, 0, 0) is None                            # M = 0


def test_na_pairs_can_leave_a_relabelling_without_a_within_value():
    """classes (a, a, b, c): the one within pair is (0, 1).  The pair (2, 3) is NA, so the relabelling (b, c, a, a),
    whose one within pair it is, has nW = 0 and no R; it is not counted as >=."""
    cells = {p: v for p, v in zip(itertools.combinations(range(4), 2), (0.9, 0.4, 0.3, 0.2, 0.1, np.nan))}
    raw = _sym(4, cells)
    res = brute_anosim(raw, [0, 0, 1, 2], 3, np.array([[1, 2, 0, 0], [0, 0, 1, 2], [0, 1, 0, 2]]))
    assert list(res["n_pairs"]) == [5, 1]
    assert list(res["nw"]) == [1, 0, 1, 1] and list(res["w2"]) == [2, 0, 2, 4]
    assert res["exact"][1][0] is None and res["n_undefined"] == 1
    # observed: within rank 1, between mean (2 + 3 + 4 + 5) / 4 = 3.5, M / 2 = 2.5: R = 1; (0, 1, 0, 2): rank 2 against 3.25
    assert res["exact"][0] == 1 and res["exact"][1][1] == 1 and res["exact"][1][2] == Fraction(1, 2)
    assert res["n_ge"] == 1 and res["pvalue"] == 0.5
    assert bits(res["perm_statistic"])[0] == 0x7FF00000000007A2


def test_ranks_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(2)
    v = np.round(rng.standard_normal(500), 1)                    # heavy ties, both zeros
    v[:3] = [-0.0, 0.0, -0.0]
    want = stats.rankdata(-(v + 0.0), "average") * 2
    assert np.array_equal(doubled_ranks(v), want.astype(np.int64)) and np.all(want == np.floor(want))


def test_statistic_helpers_agree():
    rng = np.random.default_rng(3)
    for _ in range(200):
        M = int(rng.integers(1, 2000))
        nw = int(rng.integers(0, M + 1))
        w2 = int(rng.integers(0, 2 * M * max(nw, 1)))
        assert api.anosim_statistic(M, w2, nw) == statistic(M, w2, nw)


@pytest.mark.parametrize("strata", [None, list("xxyyyxzzxy")])
def test_front_end_permutation_contract(strata):
    """With seed = 7 the labels the front end builds are the documented default_rng(7).permutation sequence."""
    codes = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 2], dtype=np.int32)
    got = api.anosim_permutations(codes, 6, seed=7, strata=strata)
    want = documented_permutations(codes, 6, 7, strata)
    assert got.dtype == np.int32 and got.shape == (6, 10) and np.array_equal(got, want)
    if strata is None:
        rng = np.random.default_rng(7)
        assert np.array_equal(got[0], rng.permutation(codes)) and np.array_equal(got[1], rng.permutation(codes))
    else:
        for st in set(strata):                                   # a stratum keeps its multiset of codes
            ix = [s for s, u in enumerate(strata) if u == st]
            assert all(sorted(row[ix]) == sorted(codes[ix]) for row in got)
    assert len({tuple(r) for r in got}) > 1
    given = np.array([[2, 2, 1, 1, 0, 0, 0, 1, 2, 2]])
    assert np.array_equal(api.anosim_permutations(codes, given), given)
    assert api.anosim_permutations(codes, 0).shape == (0, 10)
    for bad in (-1, 1000001, np.zeros((2, 9), dtype=int), np.zeros((2, 10))):
        with pytest.raises(ValueError):
            api.anosim_permutations(codes, bad)
    with pytest.raises(ValueError):
        api.anosim_permutations(codes, 3, strata=[0, 1])


def test_front_end_on_an_engine_without_anosim():
    """The fallback for checker engines: the S x S raw of the CPU oracle, ranked and summed in numpy, gives what the
    brute-force checker gives on the same raw, double for double."""
    from tests.oracle_engine import OracleEngine
    S, n = 12, 30
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[:, :6] += 2.0 * rng.standard_normal((n, 1))                # the first class shares a factor
    X[rng.random((n, S)) < 0.08] = np.nan
    X[:, 11] = 3.0                                               # constant: NA pairs
    labels = ["a"] * 6 + ["b"] * 5 + ["c"]
    names = [f"s{i}" for i in range(S)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = api.ici_kendalltau_anosim(X, labels, permutations=20, seed=7, colnames=names, engine=OracleEngine())
        full = api.ici_kendalltau(X, colnames=names, engine=OracleEngine())
        short = api.ici_kendalltau_anosim(X, labels, permutations=20, seed=7, colnames=names, engine=OracleEngine(),
                                          return_perms=False)
    codes = np.array([0] * 6 + [1] * 5 + [2], dtype=np.int32)
    ref = brute_anosim(np.asarray(full["raw"]), codes, 3, documented_permutations(codes, 20, 7))
    assert got["class_levels"] == ["a", "b", "c"] and got["n_permutations"] == 20
    assert got["n_valid"] == ref["n_pairs"][0] == 55 and got["n_na"] == ref["n_pairs"][1] == 11
    for key in ("w2", "nw", "class_w2", "class_nw"):
        assert np.array_equal(got["sums"][key], ref[key]), key
    assert got["n_ge"] == ref["n_ge"] and got["n_undefined"] == ref["n_undefined"]
    for key in ("statistic", "pvalue", "perm_statistic", "class_mean_rank", "within_mean_rank", "between_mean_rank"):
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
    assert got["statistic"] > 0 and "perm_statistic" not in short and short["statistic"] == got["statistic"]
    with pytest.raises(ValueError):
        api.ici_kendalltau_anosim(X, None, colnames=names, engine=OracleEngine())
