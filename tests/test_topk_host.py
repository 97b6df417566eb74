"""api.ici_kendalltau_topk on an engine without a topk method (the CPU oracle): the selection from the full result
(api._topk_numpy) against the brute-force checker, the padding, the tie rule, the warnings and the CSR converter."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api, formats
from tests.oracle_engine import OracleEngine
from tests.topk_checker import NA_REAL_BITS, brute_topk

KEYS = ("cor", "raw", "pvalue", "taumax", "completeness")


def _data(S=9, n=60, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, S))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X, [f"s{i}" for i in range(S)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _full(X, names, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = api.ici_kendalltau(X, colnames=names, engine=OracleEngine(), **kw)
    return [np.asarray(full[key]) for key in KEYS]


def _topk(X, names, k, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return api.ici_kendalltau_topk(X, k, colnames=names, engine=OracleEngine(), **kw)


def _assert_matches(res, ref):
    idx, vals, n_valid = ref
    assert np.array_equal(res["indices"], idx)
    assert np.array_equal(res["n_valid"], n_valid)
    for q, key in enumerate(KEYS):
        assert np.array_equal(_bits(res[key]), _bits(vals[q])), key


@pytest.mark.parametrize("perspective", ["global", "local"])
@pytest.mark.parametrize("scale_max", [True, False])
def test_topk_equals_checker_on_full_result(perspective, scale_max):
    X, names = _data()
    res = _topk(X, names, 4, perspective=perspective, scale_max=scale_max)
    _assert_matches(res, brute_topk(_full(X, names, perspective=perspective, scale_max=scale_max), 4))
    taumax = _full(X, names, perspective=perspective, scale_max=scale_max)[3]
    assert res["max_taumax"] == np.nanmax(taumax[np.triu_indices(len(names), k=1)])
    assert res["indices"].dtype == np.int32 and res["indices"].shape == (len(names), 4)


def test_constant_column_is_no_ones_partner():
    X, names = _data()
    X[:, 4] = 2.5
    S = len(names)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = api.ici_kendalltau_topk(X, S - 1, colnames=names, engine=OracleEngine())
    msgs = [str(x.message) for x in w if str(x.message) == _lib.REASON_WARNINGS[_lib.REASON_SINGLE_UNIQUE]]
    assert len(msgs) == S - 1                       # once per pair of the constant column
    assert res["n_valid"][4] == 0
    assert np.all(res["indices"][4] == -1)
    assert np.all(_bits(res["raw"][4]) == NA_REAL_BITS)
    assert not np.any(res["indices"] == 4)
    others = [c for c in range(S) if c != 4]
    assert np.all(res["n_valid"][others] == S - 2)
    assert np.all(res["indices"][others, S - 2] == -1)


def test_equal_raw_is_ordered_by_index():
    X, names = _data(S=8)
    X[:, 5] = X[:, 1]
    X[:, 6] = X[:, 1]
    S = len(names)
    res = _topk(X, names, S - 1)
    for c in (0, 2, 3, 4, 7):
        row = res["indices"][c].tolist()
        at = [row.index(j) for j in (1, 5, 6)]
        assert at == [at[0], at[0] + 1, at[0] + 2], (c, row)     # equal raw: adjacent, the smaller index first
        raws = _bits(res["raw"][c])[at]
        assert raws[0] == raws[1] == raws[2]
    assert res["indices"][1, :2].tolist() == [5, 6]
    assert res["indices"][6, :2].tolist() == [1, 5]


@pytest.mark.parametrize("k_of_s", [lambda S: 1, lambda S: S - 1, lambda S: S + 5])
def test_k_edges_and_padding(k_of_s):
    X, names = _data()
    S = len(names)
    k = k_of_s(S)
    res = _topk(X, names, k)
    _assert_matches(res, brute_topk(_full(X, names), k))
    assert np.array_equal(res["n_valid"], np.full(S, min(k, S - 1)))
    if k > S - 1:
        assert np.all(res["indices"][:, S - 1:] == -1)
        for key in KEYS:
            assert np.all(_bits(res[key])[:, S - 1:] == NA_REAL_BITS)


@pytest.mark.parametrize("k", [0, 257, 2.5, True, "3"])
def test_bad_k_is_a_value_error(k):
    X, names = _data()
    with pytest.raises(ValueError, match="`k` must be an integer in 1 .. 256"):
        api.ici_kendalltau_topk(X, k, colnames=names, engine=OracleEngine())


def test_front_end_checks_are_ici_kendalltaus():
    X, names = _data()
    with pytest.raises(ValueError, match="Colnames"):
        api.ici_kendalltau_topk(X, 2, engine=OracleEngine())
    with pytest.raises(ValueError, match="No comparisons to do"):
        api.ici_kendalltau_topk(X[:, :1], 2, colnames=names[:1], engine=OracleEngine())


def test_neighbors_are_the_names_of_indices():
    X, names = _data()
    X[:, 2] = np.nan                                    # an all-missing sample: padding in every list
    res = _topk(X, names, len(names) - 1)
    assert res["neighbors"].shape == res["indices"].shape
    for c in range(len(names)):
        for j, nm in zip(res["indices"][c], res["neighbors"][c]):
            assert nm == (names[j] if j >= 0 else None)
    assert res["n_valid"][2] == 0 and all(nm is None for nm in res["neighbors"][2])


def test_topk_to_csr():
    pytest.importorskip("scipy")
    X, names = _data()
    X[:, 2] = np.nan
    S = len(names)
    res = _topk(X, names, 3)
    for value in ("cor", "raw"):
        g = formats.topk_to_csr(res, value=value)
        assert g.shape == (S, S)
        assert g.nnz == int(res["n_valid"].sum())
        dense = g.toarray()
        for c in range(S):
            m = res["n_valid"][c]
            assert np.array_equal(np.sort(g.indices[g.indptr[c]:g.indptr[c + 1]]), np.sort(res["indices"][c, :m]))
            assert np.array_equal(dense[c, res["indices"][c, :m]], res[value][c, :m])
    with pytest.raises(ValueError):
        formats.topk_to_csr(res, value="nope")
