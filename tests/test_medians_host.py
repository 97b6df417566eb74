"""api.ici_kendalltau_medians on an engine without a class_medians method (the CPU oracle): the reduction from the
full result (api._class_medians_numpy) against the brute-force checker (tests/medians_checker.py), the checker itself
on a hand-written matrix, labels and names, the argument errors of the Python layer and the exports."""
import os
import re
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.medians_checker import NA_REAL_BITS, bits, brute_medians, class_pairs
from tests.oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA = float(np.array([NA_REAL_BITS]).view(np.float64)[0])
nan = float("nan")


def test_checker_on_a_hand_written_matrix():
    """Five samples: classes {0, 1, 2, 4} and the singleton {3}.  Pair (0, 4) is NA; sample 4's partners are then 1 and 2
    (even), sample 1 has three partners (odd) with a -0.0 in the middle, sample 0 has two."""
    raw = np.zeros((5, 5))
    cells = {(0, 1): -0.0, (0, 2): 0.5, (0, 4): nan, (1, 2): -0.25, (1, 4): 0.75, (2, 4): 0.125,
             (0, 3): 0.9, (1, 3): 0.9, (2, 3): 0.9, (3, 4): 0.9}     # (sample 3's cells: another class, never read)
    for (i, j), v in cells.items():
        raw[i, j] = raw[j, i] = v
    np.fill_diagonal(raw, 1.0)
    cor = raw / 0.5
    out5 = [cor, raw, raw, raw, raw]
    cls = np.array([0, 0, 0, 1, 0])
    med2, n_valid = brute_medians(out5, cls)
    assert n_valid.tolist() == [2, 3, 3, 0, 2]
    # sample 0: {-0.0, 0.5} -> 0.25; sample 1: {-0.25, -0.0, 0.75} -> the middle -0.0 as +0; sample 2: {-0.25, 0.125,
    # 0.5} -> 0.125; sample 3: a singleton; sample 4: {0.125, 0.75} -> 0.4375
    want_raw = np.array([0.25, 0.0, 0.125, NA, 0.4375])
    assert np.array_equal(bits(med2[1]), bits(want_raw))
    assert not np.signbit(med2[1][1]) and not np.signbit(med2[0][1])
    want_cor = np.array([0.5, 0.0, 0.25, NA, 0.875])
    assert np.array_equal(bits(med2[0]), bits(want_cor))
    # a sample whose partners are all NA: n_valid 0 and NA, as for the singleton
    raw2 = raw.copy()
    raw2[4, :4] = raw2[:4, 4] = nan
    med2b, n_valid_b = brute_medians([raw2 / 0.5, raw2, raw2, raw2, raw2], cls)
    assert n_valid_b.tolist() == [2, 2, 2, 0, 0]
    assert bits(med2b[1])[4] == NA_REAL_BITS and bits(med2b[0])[4] == NA_REAL_BITS
    assert np.array_equal(bits(med2b[1][:3]), bits(np.array([0.25, -0.125, 0.125])))
    # the package's own numpy routine states the same contract
    for r, c in ((raw, cor), (raw2, raw2 / 0.5)):
        got2, got_n = api._class_medians_numpy(c, r, cls)
        ref2, ref_n = brute_medians([c, r, r, r, r], cls)
        assert np.array_equal(bits(got2), bits(ref2)) and np.array_equal(got_n, ref_n)
    # one class (cls None): sample 3 joins in
    med2c, n_valid_c = brute_medians(out5, None)
    assert n_valid_c.tolist() == [3, 4, 4, 4, 3]
    assert med2c[1][3] == 0.9 and med2c[1][0] == 0.5


def test_class_pairs_order():
    pi, pj = class_pairs(np.array([1, 0, 1, 0, 1, 2]))
    assert list(zip(pi.tolist(), pj.tolist())) == [(1, 3), (0, 2), (0, 4), (2, 4)]
    pi, pj = class_pairs(np.zeros(4, dtype=int))
    assert list(zip(pi.tolist(), pj.tolist())) == [(a, b) for a in range(4) for b in range(a + 1, 4)]


@pytest.fixture(scope="module")
def dataset(golden_dir):
    X = np.load(os.path.join(golden_dir, "missing_dataset.npz"))["X"]
    return X, [f"S{i + 1}" for i in range(X.shape[1])]


def _medians(X, names, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return api.ici_kendalltau_medians(X, colnames=names, engine=OracleEngine(), **kw)


def _reference(X, names, cls, **kw):
    pi, pj = class_pairs(cls)
    inc = [[names[i] for i in pi], [names[j] for j in pj]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = api.ici_kendalltau(X, colnames=names, engine=OracleEngine(), include_only=inc, **kw)
    out5 = [np.asarray(full[key]) for key in ("cor", "raw", "pvalue", "taumax", "completeness")]
    tm = out5[3][pi, pj]
    return brute_medians(out5, cls), float(np.nanmax(tm))


@pytest.mark.parametrize("kw", [{}, {"scale_max": False}, {"perspective": "local"}])
def test_front_end_one_class(dataset, kw):
    X, names = dataset
    S = len(names)
    res = _medians(X, names, **kw)
    (med2, n_valid), mx = _reference(X, names, np.zeros(S, dtype=int), **kw)
    assert np.array_equal(bits(res["med_cor"]), bits(med2[0]))
    assert np.array_equal(bits(res["med_raw"]), bits(med2[1]))
    assert np.array_equal(res["n_valid"], n_valid) and np.all(n_valid == S - 1)
    assert res["max_taumax"] == mx
    assert res["sample_id"] == names and res["sample_class"] == ["all"] * S
    if not kw.get("scale_max", True):
        assert np.array_equal(bits(res["med_cor"]), bits(res["med_raw"]))


def test_front_end_interleaved_classes_with_a_singleton(dataset):
    X, names = dataset
    S = len(names)
    labels = ["b", "a", "c"] + ["a", "b"] * ((S - 3) // 2) + ["a"] * ((S - 3) % 2)     # "c": a singleton
    assert len(labels) == S and labels.count("c") == 1
    cls = np.array([{"a": 0, "b": 1, "c": 2}[v] for v in labels])
    res = _medians(X, names, sample_classes=labels)
    (med2, n_valid), mx = _reference(X, names, cls)
    assert np.array_equal(bits(res["med_cor"]), bits(med2[0]))
    assert np.array_equal(bits(res["med_raw"]), bits(med2[1]))
    assert np.array_equal(res["n_valid"], n_valid)
    assert n_valid[2] == 0 and bits(res["med_raw"])[2] == NA_REAL_BITS and bits(res["med_cor"])[2] == NA_REAL_BITS
    assert res["max_taumax"] == mx
    assert res["sample_id"] == names and res["sample_class"] == labels         # in sample order
    # the scale is the within-class maximum: with one class more pairs count
    whole = _medians(X, names)
    assert whole["max_taumax"] >= res["max_taumax"]


def test_all_singletons_is_no_error(dataset):
    X, names = dataset
    res = _medians(X[:, :4], names[:4], sample_classes=[3, 1, 2, 0])
    assert res["n_valid"].tolist() == [0, 0, 0, 0] and res["max_taumax"] == -np.inf
    assert np.all(bits(res["med_cor"]) == NA_REAL_BITS) and np.all(bits(res["med_raw"]) == NA_REAL_BITS)
    assert res["sample_class"] == [3, 1, 2, 0]


def test_argument_errors(dataset):
    X, names = dataset
    with pytest.raises(ValueError, match="`sample_classes` must give one class per column"):
        api.ici_kendalltau_medians(X, sample_classes=["a"] * 3, colnames=names, engine=OracleEngine())
    with pytest.raises(ValueError, match="Colnames"):
        api.ici_kendalltau_medians(X, engine=OracleEngine())
    with pytest.raises(ValueError, match="No comparisons to do"):
        api.ici_kendalltau_medians(X[:, :1], colnames=names[:1], engine=OracleEngine())


def test_exports():
    import icikendalltau_amd as pkg
    assert pkg.ici_kendalltau_medians is api.ici_kendalltau_medians
    src = open(os.path.join(ROOT, "include", "icikt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for nm in ("icikt_class_medians_f64", "icikt_class_medians_in", "icikt_class_medians_csc"):
        assert nm in _lib.EXPORTS
        assert re.search(rf"\bint {nm}\s*\(", src), nm
    assert os.path.join(ROOT, "icikendalltau_amd", "csrc", "icikt_medians.hip") in _lib.SOURCES
    assert hasattr(api.HipEngine, "class_medians") and hasattr(api.MultiHipEngine, "class_medians")
    assert hasattr(_lib.Context, "class_medians")
