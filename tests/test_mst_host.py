"""ici_kendalltau_mst without a GPU: the plain-numpy route of the front end (_mst_numpy), the brute-force checker
(tests/mst_checker.py) and the converters (formats.mst_to_linkage, formats.mst_cut), held against closed forms, against
each other, against a verifier that does not go through Kruskal, and against scipy's single linkage."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import api, formats
from icikendalltau_amd.api import _mst_numpy, ici_kendalltau_mst
from tests import designed_tau as dt
from tests.mst_checker import bits, brute_mst, tied_competitors, verify_forest
from tests.oracle_engine import OracleEngine


def _five(raw):
    """five planes for _mst_numpy: raw in every place (the planes are only gathered)"""
    return [raw] * 5


def _names(S):
    return [f"s{i}" for i in range(S)]


def _front(X, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ici_kendalltau_mst(X, colnames=_names(X.shape[1]), engine=OracleEngine(), **kw)


def _continuous(S, n, seed=31):
    rng = np.random.default_rng(seed + 1000 * S + n)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X


_RAW = {}


def _oracle_raw(S, n):
    """(X, raw [S, S]) of continuous data by the CPU oracle, computed once"""
    if (S, n) not in _RAW:
        X = _continuous(S, n)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            full = api.ici_kendalltau(X, colnames=_names(S), engine=OracleEngine())
        _RAW[(S, n)] = (X, np.asarray(full["raw"], dtype=np.float64), full)
    return _RAW[(S, n)]


# ---- closed forms ----------------------------------------------------------------------------------------------------

def _swaps_path(S=17, n=40):
    """positive signs, distinct k: raw[a, b] = (m - 2 |k_a - k_b|) / m, points on a line -- the tree is the path through
    the columns sorted by k, whatever the tie-break; its edges in the strict order are sorted on the integers"""
    ks = np.random.default_rng(8).permutation(n // 2 + 1)[:S]
    d = dt.swaps(S, n, seed=1, params=ks, signs=np.ones(S, dtype=np.int32))
    by_k = np.argsort(ks)
    a, b = by_k[:-1], by_k[1:]
    i, j = np.minimum(a, b), np.maximum(a, b)
    gap = np.abs(ks[a] - ks[b])
    idx = i * (2 * S - i - 1) // 2 + (j - i - 1)
    order = np.lexsort((idx, gap))                            # the smaller gap = the larger num first, then combn order
    return d, i[order].astype(np.int32), j[order].astype(np.int32), d.value(d.m - 2 * gap[order])


def test_closed_form_path_of_the_swaps_design():
    d, wi, wj, wraw = _swaps_path()
    S = d.S
    assert len(set(np.diff(np.sort(d.param)).tolist())) >= 2 and len(wi) == S - 1
    ti, tj, vals, component, n_comp = _mst_numpy(_five(d.raw), None)
    assert np.array_equal(ti, wi) and np.array_equal(tj, wj) and np.array_equal(bits(vals[1]), bits(wraw))
    assert n_comp == 1 and np.all(component == 0)
    bi, bj, bcomp, bn = brute_mst(d.raw)
    assert np.array_equal(bi, wi) and np.array_equal(bj, wj) and bn == 1 and np.all(bcomp == 0)
    verify_forest(d.raw, wi, wj, np.zeros(S, dtype=np.int32))
    res = _front(d.X)
    assert np.array_equal(res["i"], wi) and np.array_equal(res["j"], wj)
    assert np.array_equal(bits(res["raw"]), bits(wraw)) and np.array_equal(bits(res["cor"]), bits(wraw))
    assert np.all(res["taumax"] == 1.0) and res["max_taumax"] == 1.0
    assert res["n_tree"] == S - 1 and res["n_components"] == 1 and np.all(res["component"] == 0)
    assert list(res["s1"]) == [f"s{i}" for i in wi] and list(res["s2"]) == [f"s{j}" for j in wj]
    assert list(res["sample_id"]) == _names(S)


def test_identical_columns_give_the_star():
    S = 9
    raw = np.full((S, S), 1.0)
    star_i, star_j = np.zeros(S - 1, dtype=np.int32), np.arange(1, S, dtype=np.int32)
    ti, tj, _vals, component, n_comp = _mst_numpy(_five(raw), None)
    assert np.array_equal(ti, star_i) and np.array_equal(tj, star_j) and n_comp == 1 and np.all(component == 0)
    bi, bj, _c, bn = brute_mst(raw)
    assert np.array_equal(bi, star_i) and np.array_equal(bj, star_j) and bn == 1
    verify_forest(raw, star_i, star_j, np.zeros(S, dtype=np.int32))
    # -0 equals +0: a mixed-sign zero matrix is all ties too
    zeros = np.where(np.add.outer(np.arange(S), np.arange(S)) % 2 == 0, 0.0, -0.0)
    ti, tj, _vals, _c, _n = _mst_numpy(_five(zeros), None)
    bi, bj, _c, _n = brute_mst(zeros)
    assert np.array_equal(ti, star_i) and np.array_equal(tj, star_j) and np.array_equal(bi, star_i) and np.array_equal(bj, star_j)
    col = np.random.default_rng(3).standard_normal(30)
    res = _front(np.asfortranarray(np.tile(col[:, None], (1, S))))
    assert np.array_equal(res["i"], star_i) and np.array_equal(res["j"], star_j) and len(set(res["raw"].tolist())) == 1


def test_constant_and_all_nan_columns_are_singletons():
    S, n = 14, 40
    d = dt.swaps(S, n, seed=3, n_all_missing=1, n_constant=1, flip=0.0)
    lone = np.flatnonzero(d.kind != dt.VALID)
    assert len(lone) == 2
    want = np.empty(S, dtype=np.int32)                        # numbered in order of each component's smallest sample
    label = {}
    for s in range(S):
        want[s] = label.setdefault(("lone", s) if s in lone else "big", len(label))
    ti, tj, _v, component, n = _mst_numpy(_five(d.raw), None)
    for bi, bj, comp, n_comp in ((ti, tj, component, n), brute_mst(d.raw)):
        assert len(bi) == S - 3 and n_comp == 3 and np.array_equal(comp, want)
        assert not np.any(np.isin(bi, lone)) and not np.any(np.isin(bj, lone))
        verify_forest(d.raw, bi, bj, comp)
    res = _front(d.X)
    assert res["n_tree"] == S - 3 and res["n_components"] == 3 and np.array_equal(res["component"], want)
    assert res["n_tree"] + res["n_components"] == S
    with pytest.raises(ValueError, match="n_components = 3"):
        formats.mst_to_linkage(res)


# ---- the numpy route against the checker and the verifier ------------------------------------------------------------

@pytest.mark.parametrize("pct", [None, 50, 90, 99])
def test_numpy_route_against_checker_and_verifier(pct):
    S, n = 65, 40
    _X, raw, _full = _oracle_raw(S, n)
    tri = raw[np.triu_indices(S, k=1)]
    assert not np.any(np.isnan(tri))
    min_raw = None if pct is None else float(np.percentile(tri, pct))
    ti, tj, vals, component, n_comp = _mst_numpy(_five(raw), min_raw)
    bi, bj, bcomp, bn = brute_mst(raw, min_raw)
    assert np.array_equal(ti, bi) and np.array_equal(tj, bj) and np.array_equal(component, bcomp) and n_comp == bn
    assert np.array_equal(bits(vals[1]), bits(raw[ti, tj])) and np.all(np.diff(vals[1]) <= 0)
    assert verify_forest(raw, ti, tj, component, min_raw) == n_comp
    assert len(ti) + n_comp == S
    if pct is None:
        assert n_comp == 1
    if pct == 99:
        assert n_comp > 10


def test_verifier_rejects_a_wrong_forest():
    S, n = 65, 40
    _X, raw, _full = _oracle_raw(S, n)
    ti, tj, comp, _n = brute_mst(raw)
    # the star is a spanning tree, not the maximum one; a tree short of an edge leaves a candidate between two trees
    with pytest.raises(AssertionError):
        verify_forest(raw, np.zeros(S - 1, dtype=np.int32), np.arange(1, S, dtype=np.int32), comp)
    with pytest.raises(AssertionError):
        verify_forest(raw, ti[:-1], tj[:-1], comp)


def test_ties_are_broken_by_the_combn_index():
    """few rows: a few dozen distinct values among 2 080 pairs, so equal keys compete for the tree"""
    S, n = 65, 9
    _X, raw, _full = _oracle_raw(S, n)
    ti, tj, vals, component, n_comp = _mst_numpy(_five(raw), None)
    bi, bj, bcomp, bn = brute_mst(raw)
    assert tied_competitors(raw, bi, bj) >= S // 2
    assert np.array_equal(ti, bi) and np.array_equal(tj, bj) and np.array_equal(component, bcomp) and n_comp == bn
    verify_forest(raw, ti, tj, component)


# ---- the converters ---------------------------------------------------------------------------------------------------

def _result(S, n, min_raw=None):
    X, raw, _full = _oracle_raw(S, n)
    return X, raw, _front(X, min_raw=min_raw)


def _partition(labels):
    """a labelling as a canonical partition: numbered by first appearance"""
    seen, out = {}, []
    for v in np.asarray(labels).tolist():
        out.append(seen.setdefault(v, len(seen)))
    return out


def test_linkage_is_scipys_single_linkage():
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    dist = pytest.importorskip("scipy.spatial.distance")
    S, n = 130, 700
    _X, raw, res = _result(S, n)
    assert not np.any(np.isnan(raw[np.triu_indices(S, k=1)])) and res["n_components"] == 1
    D = 1.0 - raw
    np.fill_diagonal(D, 0.0)
    Zref = hier.linkage(dist.squareform(D, checks=True), "single")
    Z = formats.mst_to_linkage(res)
    assert Z.shape == (S - 1, 4) and Z.dtype == np.float64
    assert np.array_equal(bits(Z[:, 2]), bits(Zref[:, 2]))
    assert hier.is_valid_linkage(Z)
    for q in (5, 25, 50, 75, 95):
        t = float(np.percentile(Zref[:, 2], q))
        assert _partition(hier.fcluster(Z, t, "distance")) == _partition(hier.fcluster(Zref, t, "distance"))
    assert len(np.unique(Zref[:, 2])) == S - 1                # no two tree heights coincide: the merges are unique
    assert np.array_equal(Z, Zref)
    assert np.all(Z[:, 0] < Z[:, 1]) and Z[-1, 3] == S
    # by cor: the same tree, heights 1 - cor
    Zc = formats.mst_to_linkage(res, by="cor")
    assert np.array_equal(Zc[:, [0, 1, 3]], Z[:, [0, 1, 3]]) and np.array_equal(bits(Zc[:, 2]), bits(1.0 - res["cor"]))
    with pytest.raises(ValueError, match="`by`"):
        formats.mst_to_linkage(res, by="pvalue")


def test_linkage_refuses_a_forest():
    S, n = 65, 40
    _X, raw, _res = _result(S, n)
    t = float(np.percentile(raw[np.triu_indices(S, k=1)], 99))
    _X, _raw, cut = _result(S, n, min_raw=t)
    assert cut["n_components"] > 1
    with pytest.raises(ValueError, match=f"n_components = {cut['n_components']}"):
        formats.mst_to_linkage(cut)


def test_cut_gives_the_components_at_every_threshold():
    S, n = 65, 40
    _X, raw, res = _result(S, n)
    tri = raw[np.triu_indices(S, k=1)]
    cuts = [float(np.percentile(tri, q)) for q in (10, 50, 90, 99, 99.9)] + [float(tri.max()) + 0.125, -1.0]
    seen = set()
    for t in cuts:
        _bi, _bj, want, n_comp = brute_mst(raw, t)
        got = formats.mst_cut(res, t)
        assert got.dtype == np.int32 and np.array_equal(got, want), t
        assert np.array_equal(_front(_X, min_raw=t)["component"], want)
        seen.add(n_comp)
    assert 1 in seen and S in seen and len(seen) >= 4
    assert np.array_equal(formats.mst_cut(res, float(tri.max()) + 0.125), np.arange(S))
    assert np.array_equal(formats.mst_cut(res, -1.0), np.zeros(S))


# ---- the front end's argument checks ---------------------------------------------------------------------------------

def test_argument_errors():
    X = _continuous(6, 20)
    names = _names(6)
    eng = OracleEngine()
    with pytest.raises(ValueError, match="`min_raw` must not be NaN"):
        ici_kendalltau_mst(X, min_raw=float("nan"), colnames=names, engine=eng)
    with pytest.raises(ValueError, match="`min_raw` must be a number or None"):
        ici_kendalltau_mst(X, min_raw="0.5", colnames=names, engine=eng)
    with pytest.raises(ValueError, match="`min_raw` must be a number or None"):
        ici_kendalltau_mst(X, min_raw=True, colnames=names, engine=eng)
    with pytest.raises(ValueError, match="No comparisons to do"):
        ici_kendalltau_mst(X[:, :1], colnames=names[:1], engine=eng)
    import icikendalltau_amd
    assert icikendalltau_amd.ici_kendalltau_mst is ici_kendalltau_mst
    assert icikendalltau_amd.mst_to_linkage is formats.mst_to_linkage and icikendalltau_amd.mst_cut is formats.mst_cut
