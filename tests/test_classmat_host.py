"""api.ici_kendalltau_class_matrix on an engine without a class_matrix method (the CPU oracle): the reduction from the
full result (api._class_matrix_numpy) against the brute-force checker (tests/classmat_checker.py), the checker itself on
a hand-written matrix, the two identities with ici_kendalltau_medians, labels and names, nearest_class, the argument
errors of the Python layer and the exports."""
import os
import re
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.classmat_checker import NA_REAL_BITS, bits, brute_class_matrix, clear_nearest, signal_matrix
from tests.oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA = float(np.array([NA_REAL_BITS]).view(np.float64)[0])
nan = float("nan")


def test_checker_on_a_hand_written_matrix():
    """Five samples: class 0 = {0, 1, 2, 4}, class 1 = the singleton {3}, class 2 empty.  Pair (0, 4) is NA.  Column 0:
    sample 0 has two partners (even), sample 1 three (odd) with a -0.0 in the middle, sample 3 -- not a member -- all
    four (even), sample 4 two.  Column 1: one key per cell, and the singleton's own cell has none."""
    raw = np.zeros((5, 5))
    cells = {(0, 1): -0.0, (0, 2): 0.5, (0, 4): nan, (1, 2): -0.25, (1, 4): 0.75, (2, 4): 0.125,
             (0, 3): 0.3, (1, 3): -0.6, (2, 3): 0.9, (3, 4): 0.2}
    for (i, j), v in cells.items():
        raw[i, j] = raw[j, i] = v
    np.fill_diagonal(raw, 1.0)
    cor = raw / 0.5
    out5 = [cor, raw, raw, raw, raw]
    cls = np.array([0, 0, 0, 1, 0])
    med2, n_valid = brute_class_matrix(out5, cls, 3)
    assert med2.shape == (2, 5, 3) and n_valid.shape == (5, 3)
    assert n_valid.tolist() == [[2, 1, 0], [3, 1, 0], [3, 1, 0], [4, 0, 0], [2, 1, 0]]
    # column 0 -- sample 0: {-0.0, 0.5} -> 0.25; 1: {-0.25, -0.0, 0.75} -> the middle -0.0 as +0; 2: {-0.25, 0.125, 0.5}
    # -> 0.125; 3: {-0.6, 0.2, 0.3, 0.9} -> 0.25; 4: {0.125, 0.75} -> 0.4375.  Column 1: the cell with sample 3
    want_raw = np.array([[0.25, 0.3, NA], [0.0, -0.6, NA], [0.125, 0.9, NA], [0.25, NA, NA], [0.4375, 0.2, NA]])
    assert np.array_equal(bits(med2[1]), bits(want_raw))
    assert not np.signbit(med2[1][1, 0]) and not np.signbit(med2[0][1, 0])
    want_cor = np.array([[0.5, 0.3 / 0.5, NA], [0.0, -0.6 / 0.5, NA], [0.25, 0.9 / 0.5, NA],
                         [(0.2 / 0.5 + 0.3 / 0.5) * 0.5, NA, NA], [0.875, 0.2 / 0.5, NA]])
    assert np.array_equal(bits(med2[0]), bits(want_cor))
    # NA bits exactly where there is no partner: the empty class, the singleton's own cell
    assert np.array_equal(bits(med2[1]) == NA_REAL_BITS, n_valid == 0)
    # a sample whose pairs are all NA: its whole row is NA, and it is no one's partner
    raw2 = raw.copy()
    raw2[4, :4] = raw2[:4, 4] = nan
    med2b, n_valid_b = brute_class_matrix([raw2 / 0.5, raw2, raw2, raw2, raw2], cls, 3)
    assert n_valid_b.tolist() == [[2, 1, 0], [2, 1, 0], [2, 1, 0], [3, 0, 0], [0, 0, 0]]
    assert np.all(bits(med2b[:, 4, :]) == NA_REAL_BITS)
    assert np.array_equal(bits(med2b[1][:4, 0]), bits(np.array([0.25, -0.125, 0.125, 0.3])))
    # the package's own numpy routine states the same contract
    for r, c in ((raw, cor), (raw2, raw2 / 0.5)):
        got2, got_n = api._class_matrix_numpy(c, r, cls, 3)
        ref2, ref_n = brute_class_matrix([c, r, r, r, r], cls, 3)
        assert got2.shape == ref2.shape and got_n.shape == ref_n.shape
        assert np.array_equal(bits(got2), bits(ref2)) and np.array_equal(got_n, ref_n)
    # one class (cls None): a table of one column, sample 3 joins in
    med2c, n_valid_c = brute_class_matrix(out5, None, 1)
    assert n_valid_c[:, 0].tolist() == [3, 4, 4, 4, 3]
    assert med2c[1][3, 0] == 0.25 and med2c[1][0, 0] == 0.3


def test_nearest_class_ties_go_to_the_earlier_class():
    levels = ["a", "b", "c"]
    med_raw = np.array([[0.5, 0.5, 0.1],      # a tie of a and b: a
                        [0.1, 0.7, 0.7],      # a tie of b and c: b
                        [0.9, 0.2, 0.3],      # the largest cell has no partner: c
                        [NA, NA, NA],         # no cell has a partner
                        [NA, -0.4, -0.4],     # negative values, a tie behind a cell without partners: b
                        [0.0, -0.0, -1.0]])   # the two zeros are one value: a
    n_valid = np.array([[3, 3, 3], [2, 1, 1], [0, 4, 4], [0, 0, 0], [0, 2, 5], [1, 1, 1]])
    assert api._nearest_class(med_raw, n_valid, levels) == ["a", "b", "c", None, "b", "a"]


@pytest.fixture(scope="module")
def dataset(golden_dir):
    X = np.load(os.path.join(golden_dir, "missing_dataset.npz"))["X"]
    return X, [f"S{i + 1}" for i in range(X.shape[1])]


def _quiet(fn, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, engine=OracleEngine(), **kw)


def _reference(X, names, cls, n_class, **kw):
    full = _quiet(api.ici_kendalltau, X, colnames=names, **kw)
    out5 = [np.asarray(full[key]) for key in ("cor", "raw", "pvalue", "taumax", "completeness")]
    iu = np.triu_indices(len(names), k=1)
    return brute_class_matrix(out5, cls, n_class), float(np.nanmax(out5[3][iu]))


@pytest.mark.parametrize("kw", [{}, {"scale_max": False}, {"perspective": "local"}])
def test_front_end_against_the_checker_and_the_medians_entry(dataset, kw):
    X, names = dataset
    S = len(names)
    labels = ["b", "a", "c"] + ["a", "b"] * ((S - 3) // 2) + ["a"] * ((S - 3) % 2)     # "c": a singleton
    assert len(labels) == S and labels.count("c") == 1
    levels = ["a", "b", "c"]
    cls = np.array([levels.index(v) for v in labels])
    res = _quiet(api.ici_kendalltau_class_matrix, X, labels, colnames=names, **kw)
    (med2, n_valid), mx = _reference(X, names, cls, 3, **kw)
    assert res["med_cor"].shape == res["med_raw"].shape == res["n_valid"].shape == (S, 3)
    assert np.array_equal(bits(res["med_cor"]), bits(med2[0]))
    assert np.array_equal(bits(res["med_raw"]), bits(med2[1]))
    assert np.array_equal(res["n_valid"], n_valid)
    assert res["max_taumax"] == mx
    assert res["classes"] == levels and res["sample_id"] == names and res["sample_class"] == labels   # in order
    assert n_valid[2, 2] == 0 and bits(res["med_raw"])[2, 2] == NA_REAL_BITS and bits(res["med_cor"])[2, 2] == NA_REAL_BITS
    assert np.array_equal(bits(res["med_raw"]) == NA_REAL_BITS, n_valid == 0)
    if not kw.get("scale_max", True):
        assert np.array_equal(bits(res["med_cor"]), bits(res["med_raw"]))
    assert res["nearest_class"] == api._nearest_class(med2[1], n_valid, levels)
    assert len(res["nearest_class"]) == S and set(res["nearest_class"]) <= set(levels)
    # identity 1: the own-class column is the medians entry's med_raw and n_valid
    own = _quiet(api.ici_kendalltau_medians, X, sample_classes=labels, colnames=names, **kw)
    rows = np.arange(S)
    assert np.array_equal(bits(res["med_raw"][rows, cls]), bits(own["med_raw"]))
    assert np.array_equal(res["n_valid"][rows, cls], own["n_valid"])
    # identity 2: with one class both entries scale by the same maximum, and med_cor agrees too
    one = _quiet(api.ici_kendalltau_class_matrix, X, ["all"] * S, colnames=names, **kw)
    own1 = _quiet(api.ici_kendalltau_medians, X, colnames=names, **kw)
    assert one["classes"] == ["all"] and one["med_raw"].shape == (S, 1)
    assert np.array_equal(bits(one["med_raw"][:, 0]), bits(own1["med_raw"]))
    assert np.array_equal(bits(one["med_cor"][:, 0]), bits(own1["med_cor"]))
    assert np.array_equal(one["n_valid"][:, 0], own1["n_valid"]) and one["max_taumax"] == own1["max_taumax"]
    assert one["nearest_class"] == ["all"] * S


def test_all_singletons_is_no_error(dataset):
    X, names = dataset
    res = _quiet(api.ici_kendalltau_class_matrix, X[:, :4], [3, 1, 2, 0], colnames=names[:4])
    assert res["classes"] == [0, 1, 2, 3] and res["sample_class"] == [3, 1, 2, 0]
    own = np.zeros((4, 4), dtype=bool)
    own[np.arange(4), [3, 1, 2, 0]] = True
    assert np.array_equal(res["n_valid"], (~own).astype(np.int32))           # every own cell empty, every other one key
    assert np.array_equal(bits(res["med_raw"]) == NA_REAL_BITS, own)
    assert np.array_equal(bits(res["med_cor"]) == NA_REAL_BITS, own)
    assert np.isfinite(res["max_taumax"]) and None not in res["nearest_class"]
    assert all(near != lab for near, lab in zip(res["nearest_class"], res["sample_class"]))


def test_signal_matrix_gives_clear_nearest_classes():
    """The data set of the GPU front-end test (tests/test_gpu_classmat.py): on the oracle engine alone at least 90 % of
    the samples have their two best med_raw more than 1e-9 apart, so nearest_class is compared on them."""
    X, labels, names = signal_matrix()
    res = _quiet(api.ici_kendalltau_class_matrix, X, labels, colnames=names)
    clear = clear_nearest(res["med_raw"], res["n_valid"])
    print("clear", int(clear.sum()), "of", len(clear))
    assert clear.mean() >= 0.9
    # and the signal is what decides: a clear sample of a class with partners is nearest to its own class
    own_valid = np.array([res["n_valid"][s, res["classes"].index(lab)] > 0 for s, lab in enumerate(labels)])
    hit = [near == lab for near, lab in zip(res["nearest_class"], labels)]
    assert np.mean(np.asarray(hit)[clear & own_valid]) >= 0.9
    assert res["nearest_class"][17] is None and np.all(res["n_valid"][17] == 0)      # the constant column


def test_argument_errors(dataset):
    X, names = dataset
    with pytest.raises(ValueError, match="`sample_classes` must give one class per column"):
        api.ici_kendalltau_class_matrix(X, ["a"] * 3, colnames=names, engine=OracleEngine())
    with pytest.raises(ValueError, match="`sample_classes` must give one class per column"):
        api.ici_kendalltau_class_matrix(X, None, colnames=names, engine=OracleEngine())
    with pytest.raises(TypeError):
        api.ici_kendalltau_class_matrix(X, colnames=names, engine=OracleEngine())          # sample_classes is required
    with pytest.raises(ValueError, match="Colnames"):
        api.ici_kendalltau_class_matrix(X, ["a"] * len(names), engine=OracleEngine())
    with pytest.raises(ValueError, match="No comparisons to do"):
        api.ici_kendalltau_class_matrix(X[:, :1], ["a"], colnames=names[:1], engine=OracleEngine())


def test_exports():
    import icikendalltau_amd as pkg
    assert pkg.ici_kendalltau_class_matrix is api.ici_kendalltau_class_matrix
    src = open(os.path.join(ROOT, "include", "icikt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for nm in ("icikt_class_matrix_f64", "icikt_class_matrix_in", "icikt_class_matrix_csc"):
        assert nm in _lib.EXPORTS
        assert re.search(rf"\bint {nm}\s*\(", src), nm
    for f in ("icikt_classmat.hip", "icikt_capi_classmat.cpp"):
        assert os.path.join(ROOT, "icikendalltau_amd", "csrc", f) in _lib.SOURCES
    assert os.path.join(ROOT, "icikendalltau_amd", "csrc", "icikt_select.h") in _lib.HEADERS
    assert all(os.path.exists(p) for p in _lib.SOURCES + _lib.HEADERS)
    assert hasattr(api.HipEngine, "class_matrix") and hasattr(api.MultiHipEngine, "class_matrix")
    assert hasattr(_lib.Context, "class_matrix")
    assert not hasattr(OracleEngine, "class_matrix")       # (the tests above take the numpy fallback)
