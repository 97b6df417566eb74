"""api.ici_kendalltau_edges on an engine without an edges method (the CPU oracle): the selection from the full result
(api._edges_numpy) against the brute-force checker and against the reference's long data.frame, truncation, the
argument errors of the Python layer, the warnings and the COO converter."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api, formats
from tests.edges_checker import bits, brute_edges, combn_pairs
from tests.oracle_engine import OracleEngine

KEYS = ("cor", "raw", "pvalue", "taumax", "completeness")


def _data(S=9, n=60, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, S))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X, [f"s{i}" for i in range(S)]


def _full(X, names, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return api.ici_kendalltau(X, colnames=names, engine=OracleEngine(), **kw)


def _edges(X, names, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return api.ici_kendalltau_edges(X, colnames=names, engine=OracleEngine(), **kw)


def _assert_matches(res, ref, names, max_edges=None):
    ei, ej, vals, n_edges, degree = ref
    m = n_edges if max_edges is None else min(n_edges, max_edges)
    assert res["n_edges"] == n_edges
    assert np.array_equal(res["degree"], degree)
    assert np.array_equal(res["i"], ei[:m]) and np.array_equal(res["j"], ej[:m])
    assert res["i"].dtype == np.int32 and res["j"].dtype == np.int32
    assert list(res["s1"]) == [names[a] for a in ei[:m]] and list(res["s2"]) == [names[b] for b in ej[:m]]
    for q, key in enumerate(KEYS):
        assert np.array_equal(bits(res[key]), bits(vals[q][:m])), key


def test_combn_pairs_is_combn_order():
    i, j = combn_pairs(5)
    assert list(zip(i.tolist(), j.tolist())) == [(a, b) for a in range(5) for b in range(a + 1, 5)]
    assert combn_pairs(1)[0].shape == (0,)


RULES = [{}, {"min_raw": 0.05}, {"min_raw": 0.05, "absolute": True}, {"max_pvalue": 0.3}, {"min_completeness": 0.85},
         {"min_raw": -0.05, "max_pvalue": 0.8, "min_completeness": 0.8}, {"min_raw": 2.0}]


@pytest.mark.parametrize("perspective", ["global", "local"])
@pytest.mark.parametrize("scale_max", [True, False])
def test_edges_equal_checker_on_full_result(perspective, scale_max):
    X, names = _data()
    full = _full(X, names, perspective=perspective, scale_max=scale_max)
    mats5 = [np.asarray(full[key]) for key in KEYS]
    seen = set()
    for rule in RULES:
        res = _edges(X, names, perspective=perspective, scale_max=scale_max, **rule)
        _assert_matches(res, brute_edges(mats5, **rule), names)
        seen.add(res["n_edges"])
        taumax = mats5[3][np.triu_indices(len(names), k=1)]
        assert res["max_taumax"] == np.nanmax(taumax)
    assert 0 in seen and len(names) * (len(names) - 1) // 2 in seen and len(seen) >= 4   # (the rules do cut)


def test_edges_equal_the_filtered_long_frame():
    pd = pytest.importorskip("pandas")
    X, names = _data()
    long = _full(X, names, return_matrix=False)["cor"]
    assert isinstance(long, pd.DataFrame)
    at = {nm: k for k, nm in enumerate(names)}
    rows = long[long["s1"] != long["s2"]]                       # without the diagonal
    keep = rows[(rows["raw"] >= 0.05) & (rows["pvalue"] <= 0.9)]
    a = np.array([at[v] for v in keep["s1"]])
    b = np.array([at[v] for v in keep["s2"]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((hi, lo))
    res = _edges(X, names, min_raw=0.05, max_pvalue=0.9)
    assert res["n_edges"] == len(keep) > 0
    assert np.array_equal(res["i"], lo[order]) and np.array_equal(res["j"], hi[order])
    for key in KEYS:
        assert np.array_equal(bits(res[key]), bits(keep[key].to_numpy()[order])), key


def test_absolute_keeps_the_negative_tail():
    X, names = _data()
    X[:, 1::2] *= -1.0
    X[:, 4] = -X[:, 0]
    raw = np.asarray(_full(X, names)["raw"])[np.triu_indices(len(names), k=1)]
    plain = _edges(X, names, min_raw=0.1)
    both = _edges(X, names, min_raw=0.1, absolute=True)
    assert plain["n_edges"] == int(np.sum(raw >= 0.1))
    assert both["n_edges"] == int(np.sum(np.abs(raw) >= 0.1)) > plain["n_edges"]
    assert np.any(both["raw"] < 0) and not np.any(plain["raw"] < 0)


def test_explicit_max_edges_truncates_in_combn_order():
    X, names = _data()
    mats5 = [np.asarray(_full(X, names)[key]) for key in KEYS]
    ref = brute_edges(mats5, min_raw=0.0)
    assert ref[3] > 5
    for cap in (0, 1, ref[3] - 1, ref[3], ref[3] + 10):
        res = _edges(X, names, min_raw=0.0, max_edges=cap)
        _assert_matches(res, ref, names, max_edges=cap)
        assert len(res["i"]) == min(cap, ref[3])


def test_degenerate_columns_are_no_edge_endpoints():
    X, names = _data()
    X[:, 4] = 2.5
    X[:, 6] = np.nan
    S = len(names)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = api.ici_kendalltau_edges(X, colnames=names, engine=OracleEngine())
    msgs = [str(x.message) for x in w if str(x.message) == _lib.REASON_WARNINGS[_lib.REASON_SINGLE_UNIQUE]]
    assert len(msgs) >= S - 2                           # once per pair of the constant column (bar the empty one's)
    assert res["degree"][4] == 0 and res["degree"][6] == 0
    assert not np.any(np.isin(res["i"], (4, 6))) and not np.any(np.isin(res["j"], (4, 6)))
    assert res["n_edges"] == (S - 2) * (S - 3) // 2
    assert not np.any(np.isnan(res["raw"]))


@pytest.mark.parametrize("kw", [{"min_raw": "0.5"}, {"min_raw": float("nan")}, {"max_pvalue": True},
                                {"min_completeness": [0.5]}, {"max_edges": -1}, {"max_edges": 2.5},
                                {"max_edges": True}])
def test_bad_arguments_are_value_errors(kw):
    X, names = _data()
    with pytest.raises(ValueError, match="`(min_raw|max_pvalue|min_completeness|max_edges)` must"):
        api.ici_kendalltau_edges(X, colnames=names, engine=OracleEngine(), **kw)


def test_front_end_checks_are_ici_kendalltaus():
    X, names = _data()
    with pytest.raises(ValueError, match="Colnames"):
        api.ici_kendalltau_edges(X, engine=OracleEngine())
    with pytest.raises(ValueError, match="No comparisons to do"):
        api.ici_kendalltau_edges(X[:, :1], colnames=names[:1], engine=OracleEngine())


def test_edge_rule_struct():
    r = _lib.edge_rule()
    assert np.isnan(r.min_raw) and np.isnan(r.max_pvalue) and np.isnan(r.min_completeness) and r.absolute == 0
    r = _lib.edge_rule(0.25, 0.05, 0.5, True)
    assert (r.min_raw, r.max_pvalue, r.min_completeness, r.absolute) == (0.25, 0.05, 0.5, 1)


def test_exports():
    import icikendalltau_amd as pkg
    assert pkg.ici_kendalltau_edges is api.ici_kendalltau_edges and pkg.edges_to_coo is formats.edges_to_coo
    for nm in ("icikt_edges_f64", "icikt_edges_in", "icikt_edges_csc"):
        assert nm in _lib.EXPORTS


def test_edges_to_coo():
    pytest.importorskip("scipy")
    X, names = _data()
    S = len(names)
    res = _edges(X, names, min_raw=0.0)
    m = res["n_edges"]
    assert m > 0
    for value in ("cor", "raw"):
        g = formats.edges_to_coo(res, value=value)
        assert g.shape == (S, S) and g.nnz == 2 * m
        dense = g.toarray()
        assert np.array_equal(dense, dense.T) and np.all(np.diag(dense) == 0)
        assert np.array_equal(dense[res["i"], res["j"]], res[value])
        u = formats.edges_to_coo(res, value=value, symmetric=False)
        assert u.nnz == m and np.array_equal(u.toarray(), np.triu(dense))
        assert np.array_equal(np.asarray(dense != 0).sum(axis=1), res["degree"])
    empty = formats.edges_to_coo(_edges(X, names, min_raw=2.0))
    assert empty.shape == (S, S) and empty.nnz == 0
    with pytest.raises(ValueError):
        formats.edges_to_coo(res, value="nope")
