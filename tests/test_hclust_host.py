"""ici_kendalltau_hclust without a GPU: the brute-force checker (tests/hclust_checker.py) on cases worked by hand and
against scipy's linkage, the plain-numpy route of the front end (_hclust_numpy) against the checker, and the converters
(formats.hclust_to_linkage, formats.hclust_cut) against scipy."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import api, formats
from icikendalltau_amd.api import _hclust_numpy, ici_kendalltau_hclust
from tests.hclust_checker import METHODS, bits, brute_hclust, members
from tests.oracle_engine import OracleEngine

NAN = float("nan")


def _sym(S, upper):
    """a symmetric S x S matrix from {(i, j): value}, NaN on the diagonal"""
    R = np.full((S, S), NAN)
    for (i, j), v in upper.items():
        R[i, j] = R[j, i] = v
    return R


def _merges(out):
    ma, mb, msize, mraw, _component, _n = out
    return list(zip(ma.tolist(), mb.tolist(), msize.tolist(), mraw.tolist()))


# ---- the checker on cases worked by hand ---------------------------------------------------------------------------

# (0, 2) merges first.  Sample 3 is equally close to 1 and 2, so its best partner is 1; under single linkage the merged
# cluster {0, 2} inherits 2's 0.5 to sample 3, and the pair (0, 3) now TIES with (1, 3) -- and comes first in the strict
# order, because its a is smaller: 3's neighbour moves from 1 to 0 without its key changing.
_TIE = {(0, 1): 0.2, (0, 2): 0.9, (0, 3): 0.1, (1, 2): 0.3, (1, 3): 0.5, (2, 3): 0.5}


def test_worked_tie_moves_a_neighbour_to_a_smaller_slot():
    R = _sym(4, _TIE)
    out = brute_hclust(R, "single")
    assert _merges(out) == [(0, 2, 2, 0.9), (0, 3, 3, 0.5), (0, 1, 4, 0.5)]
    assert out[5] == 1 and out[4].tolist() == [0, 0, 0, 0]
    # complete: {0, 2} is 0.2 from 1 and 0.1 from 3, so (1, 3) at 0.5 merges next; the two pairs meet at the smallest cell
    assert _merges(brute_hclust(R, "complete")) == [(0, 2, 2, 0.9), (1, 3, 2, 0.5), (0, 1, 4, 0.1)]
    # average: {0, 2} is (0.2 + 0.3) / 2 from 1 and (0.1 + 0.5) / 2 from 3; then the mean of those two and (1, 2)'s, (2, 3)'s
    w01, w03 = (1.0 * 0.2 + 1.0 * 0.3) / 2.0, (1.0 * 0.1 + 1.0 * 0.5) / 2.0
    last = (1.0 * w01 + 1.0 * w03) / 2.0
    got = _merges(brute_hclust(R, "average"))
    assert got[:2] == [(0, 2, 2, 0.9), (1, 3, 2, 0.5)] and got[2][:3] == (0, 1, 4)
    assert bits(got[2][3]) == bits(last)


def test_worked_average_weights_by_size():
    """{0, 1} merges first, then takes 2; the similarity of {0, 1, 2} to 3 weights {0, 1}'s by two and 2's by one"""
    R = _sym(4, {(0, 1): 0.9, (0, 2): 0.7, (1, 2): 0.6, (0, 3): 0.1, (1, 3): 0.2, (2, 3): 0.4})
    w2 = (1.0 * 0.7 + 1.0 * 0.6) / 2.0
    w3 = (1.0 * 0.1 + 1.0 * 0.2) / 2.0
    last = (2.0 * w3 + 1.0 * 0.4) / 3.0
    got = _merges(brute_hclust(R, "average"))
    assert [m[:3] for m in got] == [(0, 1, 2), (0, 2, 3), (0, 3, 4)]
    assert [bits(m[3]) for m in got] == [bits(0.9), bits(w2), bits(last)]


@pytest.mark.parametrize("method", METHODS)
def test_worked_na_pair_blocks_a_merge_and_leaves_a_forest(method):
    """(0, 2) has no raw: {0, 1} and {2, 3} form, and no method may join them"""
    R = _sym(4, {(0, 1): 0.9, (2, 3): 0.8, (0, 3): 0.5, (1, 2): 0.5, (1, 3): 0.5})
    ma, mb, msize, mraw, component, n_comp = brute_hclust(R, method)
    assert _merges((ma, mb, msize, mraw, component, n_comp)) == [(0, 1, 2, 0.9), (2, 3, 2, 0.8)]
    assert n_comp == 2 and component.tolist() == [0, 0, 1, 1] and len(ma) + n_comp == 4


def test_worked_min_raw_stops_early():
    R = _sym(4, _TIE)
    for method in METHODS:
        out = brute_hclust(R, method, 0.6)
        assert _merges(out) == [(0, 2, 2, 0.9)] and out[5] == 3 and out[4].tolist() == [0, 1, 0, 2]
        assert brute_hclust(R, method, 0.95)[5] == 4 and len(brute_hclust(R, method, 0.95)[0]) == 0
        assert len(brute_hclust(R, method, -1.0)[0]) == 3 and len(brute_hclust(R, method, NAN)[0]) == 3
    assert _merges(brute_hclust(R, "single", 0.5)) == [(0, 2, 2, 0.9), (0, 3, 3, 0.5), (0, 1, 4, 0.5)]   # 0.5 >= 0.5


def test_worked_one_and_two_samples():
    for method in METHODS:
        out = brute_hclust(np.full((1, 1), NAN), method)
        assert len(out[0]) == 0 and out[4].tolist() == [0] and out[5] == 1
        out = brute_hclust(_sym(2, {(0, 1): -0.25}), method)
        assert _merges(out) == [(0, 1, 2, -0.25)] and out[5] == 1
        out = brute_hclust(_sym(2, {}), method)
        assert len(out[0]) == 0 and out[4].tolist() == [0, 1] and out[5] == 2
        out = brute_hclust(_sym(2, {(0, 1): -0.0}), method)              # -0 is +0
        assert bits(out[3]).tolist() == bits([0.0]).tolist()


# ---- the checker against scipy -------------------------------------------------------------------------------------

def _uniform(S, seed):
    rng = np.random.default_rng(1000 * S + seed)
    R = np.full((S, S), NAN)
    iu = np.triu_indices(S, k=1)
    R[iu] = rng.uniform(-1.0, 1.0, len(iu[0]))
    R[(iu[1], iu[0])] = R[iu]
    return R


def _scipy_members(Z, S):
    sets = [frozenset([s]) for s in range(S)]
    for row in Z:
        sets.append(sets[int(row[0])] | sets[int(row[1])])
    return sets[S:]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("S", [2, 3, 65, 130])
def test_checker_against_scipy_linkage(S, seed):
    """Tie-free similarities: scipy's linkage on 1 - raw makes the same clusters in the same order.  1 - x is monotone,
    so complete and single heights -- a maximum or minimum of the cells 1 - raw -- are bitwise 1 - (the checker's raw).
    scipy averages 1 - raw where the rule averages raw: each of at most S - 1 updates rounds three times, (S - 1) x 3 x
    2^-53 < 5e-14 at S = 130, held to 1e-12."""
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    dist = pytest.importorskip("scipy.spatial.distance")
    R = _uniform(S, seed)
    tri = R[np.triu_indices(S, k=1)]
    assert len(np.unique(tri)) == len(tri), "the similarities are not distinct"
    y = dist.squareform(1.0 - np.where(np.isnan(R), 1.0, R), checks=False)
    for method in METHODS:
        ma, mb, msize, mraw, component, n_comp = brute_hclust(R, method)
        Z = hier.linkage(y, method)
        assert len(ma) == S - 1 and n_comp == 1
        assert members(ma, mb, S) == _scipy_members(Z, S), method
        assert np.array_equal(msize, Z[:, 3].astype(np.int32))
        err = float(np.max(np.abs((1.0 - mraw) - Z[:, 2])))
        print(method, S, seed, "largest height difference", err)
        if method == "average":
            assert err <= 1e-12
        else:
            assert np.array_equal(bits(1.0 - mraw), bits(Z[:, 2])), method


# ---- the numpy route of the front end against the checker ----------------------------------------------------------

def _tied_with_na(S, seed):
    """similarities on a grid of 21 values (ties decide most steps), some pairs without one, some -0"""
    rng = np.random.default_rng(77 + seed)
    R = np.full((S, S), NAN)
    iu = np.triu_indices(S, k=1)
    v = rng.integers(-10, 11, len(iu[0])) / 10.0
    v[v == 0.0] = -0.0
    v[rng.random(len(v)) < 0.03] = NAN
    R[iu] = v
    R[(iu[1], iu[0])] = R[iu]
    return R


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("S", [1, 2, 7, 40])
def test_numpy_route_equals_the_checker(S, method):
    for seed in range(3):
        R = _tied_with_na(S, seed)
        tri = R[np.triu_indices(S, k=1)]
        for min_raw in (None, 0.35, float(np.nanmax(tri)) + 1.0 if S > 1 and not np.all(np.isnan(tri)) else 2.0):
            want = brute_hclust(R, method, min_raw)
            got = _hclust_numpy([R] * 5, method, min_raw)
            for q in (0, 1, 2, 4):
                assert np.array_equal(got[q], want[q]) and got[q].dtype == np.int32, (q, seed, min_raw)
            assert np.array_equal(bits(got[3]), bits(want[3])) and got[5] == want[5]
            assert len(got[0]) + got[5] == S


def test_front_end_on_the_cpu_engine():
    from tests import designed_tau as dt
    S, n = 14, 40
    d = dt.swaps(S, n, seed=3, n_all_missing=1, n_constant=1)
    names = [f"s{i}" for i in range(S)]
    for method in METHODS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = ici_kendalltau_hclust(d.X, method=method, colnames=names, engine=OracleEngine())
            full = api.ici_kendalltau(d.X, colnames=names, engine=OracleEngine())
        want = brute_hclust(np.asarray(full["raw"]), method)
        assert np.array_equal(res["merge_a"], want[0]) and np.array_equal(res["merge_b"], want[1])
        assert np.array_equal(res["size"], want[2]) and np.array_equal(bits(res["raw"]), bits(want[3]))
        assert np.array_equal(res["component"], want[4]) and res["n_components"] == want[5] == 3
        assert res["n_merges"] == S - 3 and res["method"] == method and list(res["sample_id"]) == names
        assert np.array_equal(bits(res["cor"]), bits(res["raw"] / res["max_taumax"]))
        with pytest.raises(ValueError, match="n_components = 3"):
            formats.hclust_to_linkage(res)
    with pytest.raises(ValueError, match="method"):
        ici_kendalltau_hclust(d.X, method="ward", colnames=names, engine=OracleEngine())


# ---- formats ---------------------------------------------------------------------------------------------------------

def _result(R, method, min_raw=None):
    ma, mb, msize, mraw, component, n_comp = brute_hclust(R, method, min_raw)
    return {"merge_a": ma, "merge_b": mb, "size": msize, "raw": mraw, "cor": mraw * 0.5, "n_merges": len(ma),
            "component": component, "n_components": n_comp}


def _canonical(labels):
    seen = {}
    return [seen.setdefault(int(v), len(seen)) for v in labels]


@pytest.mark.parametrize("method", METHODS)
def test_linkage_matrix_is_scipys(method):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    dist = pytest.importorskip("scipy.spatial.distance")
    S = 65
    R = _uniform(S, 5)
    res = _result(R, method)
    Z = formats.hclust_to_linkage(res)
    assert Z.shape == (S - 1, 4) and Z.dtype == np.float64 and hier.is_valid_linkage(Z, throw=True)
    assert np.array_equal(bits(Z[:, 2]), bits(1.0 - res["raw"]))
    assert np.array_equal(bits(formats.hclust_to_linkage(res, by="cor")[:, 2]), bits(1.0 - res["cor"]))
    want = hier.linkage(dist.squareform(1.0 - np.where(np.isnan(R), 1.0, R), checks=False), method)
    assert np.array_equal(Z[:, [0, 1, 3]], want[:, [0, 1, 3]])
    assert np.array_equal(hier.leaves_list(Z), hier.leaves_list(want))
    assert hier.dendrogram(Z, no_plot=True)["leaves"] == hier.dendrogram(want, no_plot=True)["leaves"]
    # the clusters at a similarity between two merges: fcluster at the distance 1 - t, hclust_cut, and a stopped run
    for k in (0, 1, S // 2, S - 3, S - 2):
        lo = res["raw"][k + 1] if k + 1 < S - 1 else res["raw"][k] - 0.25
        t = 0.5 * (float(res["raw"][k]) + float(lo))
        assert lo < t < res["raw"][k]
        flat = hier.fcluster(Z, 1.0 - t, criterion="distance")
        cut = formats.hclust_cut(res, t)
        assert cut.dtype == np.int32 and _canonical(cut) == _canonical(flat) and len(set(cut.tolist())) == S - 1 - k
        assert np.array_equal(cut, brute_hclust(R, method, t)[4])
    assert np.array_equal(formats.hclust_cut(res, 2.0), np.arange(S))
    assert np.array_equal(formats.hclust_cut(res, -1.0), np.zeros(S))
    with pytest.raises(ValueError, match="by"):
        formats.hclust_to_linkage(res, by="pvalue")


def test_forest_is_refused_by_name():
    R = _sym(4, {(0, 1): 0.9, (2, 3): 0.8, (0, 3): 0.5, (1, 2): 0.5, (1, 3): 0.5})
    res = _result(R, "complete")
    with pytest.raises(ValueError, match="n_components = 2"):
        formats.hclust_to_linkage(res)
    assert formats.hclust_cut(res, 0.85).tolist() == [0, 0, 1, 2]
    assert formats.hclust_cut(res, 0.0).tolist() == [0, 0, 1, 1]
    stopped = _result(_sym(4, _TIE), "single", 0.6)
    with pytest.raises(ValueError, match="n_components = 3"):
        formats.hclust_to_linkage(stopped)
