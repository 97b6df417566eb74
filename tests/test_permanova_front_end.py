"""ici_kendalltau_permanova's front end on a stub engine, as tests/test_select_front_end.py pins the ten other selection
entries: a HipEngine without a context whose `permanova` records its arguments and answers a canned tuple of the shapes
Context.permanova's docstring gives.  No device, no library.  What is pinned: the argument checks; that a matrix the
context can read reaches the engine as the same object and a long global_na list is applied on the host (_on_device);
that an engine without the method goes through the full matrix (_from_full) and builds the same dict; the dict's keys
and types; the warnings."""
import inspect
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.oracle_engine import OracleEngine
from tests.permanova_checker import bits, na_real
from tests.test_select_front_end import CLASSES, NAMES, RCOUNTS, S, _matrix

KEYS = ["statistic", "r2", "pvalue", "ss_total", "ss_within", "ss_among", "df_among", "df_within", "n_permutations",
        "n_ge", "n_undefined", "perm_statistic", "n_valid", "n_na", "class_levels", "class_size", "class_ss", "sums",
        "sample_id", "max_taumax", "run_time"]
Q_ONE = 1 << 50                # q of a pair with raw = 0: a squared dissimilarity of 1


def _stub(rcounts=(0, 0, 0, 0, 0), n_na=0):
    """CLASSES = a a b b b.  Every pair has q = 2^50: Q = 10 q, the observed labelling has A = (1, 3) q, and so has every
    labelling with those class sizes"""
    sig = inspect.signature(api.HipEngine.permanova)
    calls = []

    def record(self, *args, **kw):
        bound = sig.bind(self, *args, **kw)
        bound.apply_defaults()
        a = dict(bound.arguments)
        calls.append(a)
        labs = np.vstack([np.asarray(a["cls"])[None, :], np.asarray(a["perm_cls"]).reshape(-1, S)])
        class_q = np.zeros((labs.shape[0], a["n_class"]), dtype=object)
        if n_na == 0:
            for l, lab in enumerate(labs):
                for c, n in enumerate(np.bincount(lab, minlength=a["n_class"])):
                    class_q[l, c] = int(n) * (int(n) - 1) // 2 * Q_ONE
        return (np.array([10 - n_na, n_na], np.int64), (10 - n_na) * Q_ONE, class_q, 0.5,
                np.asarray(rcounts, dtype=np.int64))

    eng = object.__new__(type("StubEngine", (api.HipEngine,), {"permanova": record}))
    eng.calls = calls
    return eng


def _run(eng, X=None, names=NAMES, classes=CLASSES, **kw):
    kw.setdefault("permutations", 3)
    kw.setdefault("seed", 1)
    return api.ici_kendalltau_permanova(_matrix() if X is None else X, classes, colnames=names, engine=eng, **kw)


def test_it_is_exported():
    import icikendalltau_amd
    assert icikendalltau_amd.ici_kendalltau_permanova is api.ici_kendalltau_permanova


def test_a_readable_matrix_reaches_the_engine_as_it_is():
    X = _matrix(np.float32)
    gna = (float("nan"), 7.0)
    eng = _stub()
    res = _run(eng, X, global_na=gna)
    assert len(eng.calls) == 1
    call = eng.calls[0]
    assert call["data_matrix"] is X and call["global_na"] is gna
    assert call["flags"] == 0 and not isinstance(call["flags"], bool)
    assert call["n_class"] == 2 and call["cls"].dtype == np.int32 and list(call["cls"]) == [0, 0, 1, 1, 1]
    assert call["perm_cls"].dtype == np.int32 and call["perm_cls"].shape == (3, S)
    assert np.array_equal(call["perm_cls"], api.anosim_permutations(call["cls"], 3, 1))   # ANOSIM's labellings
    assert isinstance(res["run_time"], float) and res["run_time"] >= 0.0 and res["max_taumax"] == 0.5


def test_a_long_global_na_list_is_applied_on_the_host():
    X = _matrix(np.float64)
    gna = tuple(float(v) for v in range(_lib.MASK_VALS + 3))
    eng = _stub()
    _run(eng, X, global_na=gna)
    M = eng.calls[0]["data_matrix"]
    assert isinstance(M, np.ndarray) and M.dtype == np.float64 and M.shape == X.shape
    assert np.array_equal(np.isnan(M), np.isin(X, gna))
    assert len(eng.calls[0]["global_na"]) == 1 and math.isnan(eng.calls[0]["global_na"][0])


def test_keys_types_and_values():
    res = _run(_stub())
    assert list(res) == KEYS
    # SS_T = 10 / 5 = 2, SS_W = 1 / 2 + 3 / 3 = 3 / 2, SS_A = 1 / 2; F = (1 / 2 / 1) / (3 / 2 / 3) = 1; R2 = 1 / 4
    assert res["statistic"] == 1.0 and res["r2"] == 0.25
    assert (res["ss_total"], res["ss_within"], res["ss_among"]) == (2.0, 1.5, 0.5)
    assert (res["df_among"], res["df_within"]) == (1, 3)
    assert res["n_permutations"] == 3 and res["n_ge"] == 3 and res["n_undefined"] == 0 and res["pvalue"] == 1.0
    assert res["perm_statistic"].dtype == np.float64 and list(res["perm_statistic"]) == [1.0, 1.0, 1.0]
    assert (res["n_valid"], res["n_na"]) == (10, 0)
    assert res["class_levels"] == ["a", "b"] and res["sample_id"] == NAMES
    assert res["class_size"].dtype == np.int64 and list(res["class_size"]) == [2, 3]
    assert res["class_ss"].dtype == np.float64 and list(res["class_ss"]) == [0.5, 1.0]
    assert res["sums"]["q_total"] == 10 * Q_ONE and isinstance(res["sums"]["q_total"], int)
    assert res["sums"]["class_q"].shape == (4, 2) and res["sums"]["class_q"].dtype == object
    assert all(isinstance(v, int) for v in res["sums"]["class_q"].ravel())
    for key in ("statistic", "r2", "pvalue", "ss_total", "ss_within", "ss_among", "max_taumax", "run_time"):
        assert isinstance(res[key], float), key
    for key in ("df_among", "df_within", "n_permutations", "n_ge", "n_undefined", "n_valid", "n_na"):
        assert isinstance(res[key], int) and not isinstance(res[key], bool), key
    short = _run(_stub(), return_perms=False)
    assert list(short) == [k for k in KEYS if k != "perm_statistic"] and short["statistic"] == 1.0


def test_supplied_labellings_with_other_sizes_go_through_f():
    # a a a a b has other class sizes: A = (6, 0) q, SS_W = 6 / 4, the observed 3 / 2, and with the same C' and S the
    # same F = 1, which counts as >=; a b a b b has the observed sizes and is compared by SS_W; all a has C' = 1: no F
    perms = np.array([[0, 0, 0, 0, 1], [0, 1, 0, 1, 1]], dtype=np.int64)
    res = _run(_stub(), permutations=perms)
    assert res["n_permutations"] == 2 and res["n_ge"] == 2 and res["n_undefined"] == 0
    assert bits(res["perm_statistic"]).tolist() == bits([1.0, 1.0]).tolist()
    res = _run(_stub(), permutations=np.zeros((1, S), dtype=np.int32))
    assert res["n_ge"] == 0 and res["n_undefined"] == 1 and bits(res["perm_statistic"])[0] == bits(na_real())[0]
    assert res["pvalue"] == float(Fraction(1, 2))


def test_one_warning_per_pair_of_reasons_2_to_4():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        _run(_stub(RCOUNTS))
    want = [_lib.REASON_WARNINGS[code] for code in (2, 3, 4) for _ in range(RCOUNTS[code])]
    assert [str(x.message) for x in w] == want and all(x.category is RuntimeWarning for x in w)


def test_na_pairs_warn_once_and_give_na():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = _run(_stub(n_na=4))
    assert len(w) == 1 and w[0].category is RuntimeWarning
    text = str(w[0].message)
    assert "4" in text and "ici_kendalltau_medians" in text and "n_valid" in text
    assert list(res) == KEYS
    na = bits(na_real())[0]
    for key in ("statistic", "r2", "pvalue", "ss_total", "ss_within", "ss_among"):
        assert bits(res[key])[0] == na, key
    assert np.all(bits(res["perm_statistic"]) == na) and np.all(bits(res["class_ss"]) == na)
    assert (res["n_valid"], res["n_na"], res["n_ge"], res["n_undefined"]) == (6, 4, 0, 3)
    assert (res["df_among"], res["df_within"]) == (1, 3)
    assert not res["sums"]["class_q"].any()


def test_argument_checks_come_before_the_engine(monkeypatch):
    eng = _stub()
    with pytest.raises(ValueError, match="No comparisons to do"):
        _run(eng, _matrix()[:, :1], names=["s0"], classes=["a"])
    with pytest.raises(ValueError, match="`sample_classes` must give one class per column"):
        _run(eng, classes=None)
    with pytest.raises(ValueError, match="`permutations` must be in 0"):
        _run(eng, permutations=-1)
    with pytest.raises(ValueError, match="`permutations` must be a count or an integer array"):
        _run(eng, permutations=np.zeros((2, S + 1), dtype=np.int32))
    with pytest.raises(ValueError, match="class code outside 0 .. n_class - 1"):
        _run(eng, permutations=np.full((2, S), 2, dtype=np.int32))
    with pytest.raises(ValueError, match="`strata` must give one stratum per column"):
        _run(eng, strata=["x"] * (S + 1))
    monkeypatch.setattr(_lib, "PERMANOVA_MAX_CELLS", 7)
    with pytest.raises(ValueError, match="at most 7"):
        _run(eng, permutations=3)                 # (1 + 3) x 2 cells
    assert eng.calls == []


def test_an_engine_without_the_method_returns_the_same_keys():
    assert not hasattr(OracleEngine(), "permanova")
    X = _matrix(np.float64)
    X[3, 1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fallback = _run(OracleEngine(), X)
    device = _run(_stub(), X)
    assert list(fallback) == list(device) == KEYS
    assert isinstance(fallback["run_time"], float) and fallback["run_time"] >= 0.0
    for key in device:
        assert type(fallback[key]) is type(device[key]), key
        if isinstance(device[key], np.ndarray):
            assert fallback[key].dtype == device[key].dtype and fallback[key].shape == device[key].shape, key
    assert fallback["sums"]["class_q"].dtype == object and isinstance(fallback["sums"]["q_total"], int)
