"""The front end the ten selection entries of icikendalltau_amd.api share (topk, cross, edges, medians, class_matrix,
quantiles, padjust, mst, hclust, anosim), entry by entry on a stub: a HipEngine without a context whose one method
records its arguments and answers a canned tuple of the shapes Context's docstrings give.  No device, no library.
What is pinned: a matrix the context can read reaches the engine as the same object; a global_na list longer than the
device rule is applied on the host; one warning per pair of reasons 2-4; the refusal of a matrix without a pair; the
one retry of edges and padjust when the count exceeds the room; and that the numpy route of an engine without the
method returns the same keys in the same order."""
import inspect
import math
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.oracle_engine import OracleEngine

N_FEAT, S = 12, 5
NAMES = [f"s{i}" for i in range(S)]
CLASSES = ["a", "a", "b", "b", "b"]
RCOUNTS = [0, 0, 2, 1, 3]


def _matrix(dtype=np.float32):
    rng = np.random.default_rng(11)
    return np.ascontiguousarray(rng.integers(0, 60, size=(N_FEAT, S)).astype(dtype))   # row-major


def _f(shape, value=0.25):
    return np.full(shape, value, dtype=np.float64)


# -- what each engine method answers: a well-formed tuple without reason_counts, from its bound arguments ------------
def _topk(a):
    n, k = a["data_matrix"].shape[1], a["k"]
    return np.zeros((n, k), np.int32), _f((5, n, k)), np.full(n, k, np.int32), 0.5


def _cross(a):
    sq, sr, k = a["query"].shape[1], a["reference"].shape[1], a["k"]
    return (_f((5, sq, sr)) if a["want_matrix"] else None, None if k is None else np.zeros((sq, k), np.int32),
            None if k is None else _f((5, sq, k)), None if k is None else np.full(sq, k, np.int32), 0.5)


def _edges(a):
    n, m = a["data_matrix"].shape[1], min(a["max_edges"], 7)
    return np.zeros(m, np.int32), np.ones(m, np.int32), _f((5, m)), 7, np.zeros(n, np.int64), 0.5


def _class_medians(a):
    n = a["data_matrix"].shape[1]
    return _f((2, n)), np.ones(n, np.int32), 0.5


def _class_matrix(a):
    n, c = a["data_matrix"].shape[1], a["n_class"]
    return _f((2, n, c)), np.ones((n, c), np.int32), 0.5


def _quantiles(a):
    g, p, b = (1 if a["cls"] is None else 3), len(a["probs"]), len(a["breaks"]) - 1
    return (_f((2, g, p)), _f((g, p, 2)), np.ones(g, np.int64), np.zeros(g, np.int64), np.zeros((g, b), np.int64),
            np.zeros((g, 2), np.int64), 0.5)


def _padjust(a):
    t, n_alpha = min(a["max_table"], 6), len(a["alpha"])
    return (np.array([10, 0], np.int64), np.full(n_alpha, 6, np.int64), _f(n_alpha, 0.01), _f((2, t), 0.01), 6, 0.5)


def _mst(a):
    n = a["data_matrix"].shape[1]
    m = n - 1
    return (np.zeros(m, np.int32), np.arange(1, n, dtype=np.int32), _f((5, m)), np.zeros(n, np.int32), 1, 2, 0.5)


def _hclust(a):
    n = a["data_matrix"].shape[1]
    m = n - 1
    return (np.zeros(m, np.int32), np.arange(1, n, dtype=np.int32), np.arange(2, n + 1, dtype=np.int32), _f(m), _f(m),
            np.zeros(n, np.int32), 1, 0.5)


def _anosim(a):
    n_lab, c = 1 + len(a["perm_cls"]), a["n_class"]
    return (np.array([10, 0], np.int64), np.full(n_lab, 40, np.int64), np.full(n_lab, 4, np.int64), 1, 0,
            np.full(c, 20, np.int64), np.full(c, 2, np.int64), 0.5)


# name -> (engine method, its answer, the api call: (engine, matrix, names, classes, **kw) -> dict)
ENTRIES = {
    "topk": ("topk", _topk, lambda e, X, nm, cl, **kw: api.ici_kendalltau_topk(X, 2, colnames=nm, engine=e, **kw)),
    "cross": ("cross", _cross, lambda e, X, nm, cl, **kw: api.ici_kendalltau_cross(
        X, X, k=2, query_names=nm, reference_names=nm, engine=e, **kw)),
    "edges": ("edges", _edges, lambda e, X, nm, cl, **kw: api.ici_kendalltau_edges(
        X, min_raw=-1.0, colnames=nm, engine=e, **kw)),
    "medians": ("class_medians", _class_medians, lambda e, X, nm, cl, **kw: api.ici_kendalltau_medians(
        X, cl, colnames=nm, engine=e, **kw)),
    "class_matrix": ("class_matrix", _class_matrix, lambda e, X, nm, cl, **kw: api.ici_kendalltau_class_matrix(
        X, cl, colnames=nm, engine=e, **kw)),
    "quantiles": ("quantiles", _quantiles, lambda e, X, nm, cl, **kw: api.ici_kendalltau_quantiles(
        X, probs=(0.5, 0.9), breaks=4, sample_classes=cl, colnames=nm, engine=e, **kw)),
    "padjust": ("padjust", _padjust, lambda e, X, nm, cl, **kw: api.ici_kendalltau_padjust(
        X, alpha=(0.05, 1.0), colnames=nm, engine=e, **kw)),
    "mst": ("mst", _mst, lambda e, X, nm, cl, **kw: api.ici_kendalltau_mst(X, colnames=nm, engine=e, **kw)),
    "hclust": ("hclust", _hclust, lambda e, X, nm, cl, **kw: api.ici_kendalltau_hclust(
        X, "average", colnames=nm, engine=e, **kw)),
    "anosim": ("anosim", _anosim, lambda e, X, nm, cl, **kw: api.ici_kendalltau_anosim(
        X, cl, permutations=3, seed=1, colnames=nm, engine=e, **kw)),
}
ALL = sorted(ENTRIES)
MATRIX_ARGS = {"cross": ("query", "reference")}


def _stub(entry, rcounts=(0, 0, 0, 0, 0)):
    """A HipEngine that was never initialised (no context, no device) whose `entry` method records its arguments as
    HipEngine's own signature binds them."""
    method, answer, _call = ENTRIES[entry]
    sig = inspect.signature(getattr(api.HipEngine, method))
    calls = []

    def record(self, *args, **kw):
        bound = sig.bind(self, *args, **kw)
        bound.apply_defaults()
        calls.append(dict(bound.arguments))
        return (*answer(calls[-1]), np.asarray(rcounts, dtype=np.int64))

    eng = object.__new__(type("StubEngine", (api.HipEngine,), {method: record}))
    eng.calls = calls
    return eng


def _run(entry, eng, X=None, names=NAMES, classes=CLASSES, **kw):
    return ENTRIES[entry][2](eng, _matrix() if X is None else X, names, classes, **kw)


def _matrices(entry, call):
    return [call[k] for k in MATRIX_ARGS.get(entry, ("data_matrix",))]


@pytest.mark.parametrize("entry", ALL)
def test_a_readable_matrix_reaches_the_engine_as_it_is(entry):
    X = _matrix(np.float32)
    gna = (float("nan"), 7.0)
    eng = _stub(entry)
    res = _run(entry, eng, X, global_na=gna)
    assert len(eng.calls) == 1
    call = eng.calls[0]
    assert all(M is X for M in _matrices(entry, call))
    assert call["global_na"] is gna
    assert call["flags"] == 0 and not isinstance(call["flags"], bool)
    assert isinstance(res["run_time"], float) and res["run_time"] >= 0.0
    assert res["max_taumax"] == 0.5


@pytest.mark.parametrize("entry", ALL)
def test_a_long_global_na_list_is_applied_on_the_host(entry):
    X = _matrix(np.float64)
    gna = tuple(float(v) for v in range(_lib.MASK_VALS + 3))
    assert api._host_masks(gna)
    eng = _stub(entry)
    _run(entry, eng, X, global_na=gna)
    assert len(eng.calls) == 1
    call = eng.calls[0]
    for M in _matrices(entry, call):
        assert isinstance(M, np.ndarray) and M.dtype == np.float64 and M.shape == X.shape
        assert np.array_equal(np.isnan(M), np.isin(X, gna))
        assert np.array_equal(M[~np.isnan(M)], X[~np.isin(X, gna)])
    assert len(call["global_na"]) == 1 and math.isnan(call["global_na"][0])
    assert isinstance(call["global_na"], tuple)


@pytest.mark.parametrize("entry", ALL)
def test_one_warning_per_pair_of_reasons_2_to_4(entry):
    eng = _stub(entry, RCOUNTS)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        _run(entry, eng)
    want = [_lib.REASON_WARNINGS[code] for code in (2, 3, 4) for _ in range(RCOUNTS[code])]
    assert len(w) == 6
    assert [str(x.message) for x in w] == want
    assert all(x.category is RuntimeWarning for x in w)


@pytest.mark.parametrize("entry", [e for e in ALL if e != "cross"])
def test_a_matrix_of_one_sample_is_refused_before_the_engine(entry):
    eng = _stub(entry)
    with pytest.raises(ValueError, match="No comparisons to do. Check the list of column names in `include_only` vs "
                                         "those in the samples."):
        _run(entry, eng, _matrix()[:, :1], names=["s0"], classes=["a"])
    assert eng.calls == []


def test_cross_with_an_empty_query_returns_empty_tables():
    X = _matrix()
    eng = _stub("cross")
    res = api.ici_kendalltau_cross(X[:, :0], X, k=2, query_names=[], reference_names=NAMES, engine=eng)
    assert np.asarray(res["raw"]).shape == (0, S) and res["indices"].shape == (0, 2)
    assert res["neighbors"].shape == (0, 2) and res["n_valid"].shape == (0,)
    assert res["query_names"] == [] and res["reference_names"] == NAMES
    res = api.ici_kendalltau_cross(X[:, :0], X, k=2, query_names=[], reference_names=NAMES, engine=OracleEngine())
    assert np.asarray(res["raw"]).shape == (0, S) and res["indices"].shape == (0, 2)
    assert res["max_taumax"] == -np.inf and res["run_time"] == 0.0


RETRY = {"edges": ("max_edges", "n_edges", 7, ("EDGES_DEFAULT_CAPACITY", "EDGES_CAPACITY_PER_SAMPLE")),
         "padjust": ("max_table", "n_table", 6, ("PADJUST_DEFAULT_TABLE",))}


@pytest.mark.parametrize("entry", sorted(RETRY))
def test_one_retry_when_the_count_exceeds_the_room(entry, monkeypatch):
    limit, count_key, count, capacities = RETRY[entry]
    monkeypatch.setattr(api, capacities[0], 2)           # the first call offers room for 2
    for name in capacities[1:]:
        monkeypatch.setattr(api, name, 0)
    eng = _stub(entry)
    res = _run(entry, eng, **{limit: None})
    assert [c[limit] for c in eng.calls] == [2, count]   # the second call's room is the reported count
    assert all(c["data_matrix"] is eng.calls[0]["data_matrix"] for c in eng.calls)
    assert isinstance(res["run_time"], float) and res["run_time"] >= 0.0
    assert res[count_key] == count
    assert len(res["raw" if entry == "edges" else "table_p"]) == count
    eng = _stub(entry)
    res = _run(entry, eng, **{limit: 3})
    assert [c[limit] for c in eng.calls] == [3]          # an explicit limit truncates: one call
    assert res[count_key] == count
    assert len(res["raw" if entry == "edges" else "table_p"]) == 3


@pytest.mark.parametrize("entry", ALL)
def test_an_engine_without_the_method_returns_the_same_keys(entry):
    """The numpy route (the CPU oracle has none of the ten methods) and the device route build the same dict."""
    assert not hasattr(OracleEngine(), ENTRIES[entry][0])
    X = _matrix(np.float64)
    X[3, 1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fallback = _run(entry, OracleEngine(), X)
    device = _run(entry, _stub(entry), X)
    assert list(fallback) == list(device)
    assert isinstance(fallback["run_time"], float) and fallback["run_time"] >= 0.0
    for key in device:
        if isinstance(device[key], np.ndarray):
            assert isinstance(fallback[key], np.ndarray) and fallback[key].ndim == device[key].ndim, key
