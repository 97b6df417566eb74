"""api.prepare_reference / PreparedReference and the class tables of api.ici_kendalltau_cross on an engine without a
prepared reference (the CPU oracle): the PreparedReference holds the host matrix and every batch takes the numpy route.
The class tables are checked against the plain-loop checker (tests/cross_class_checker.py), which is itself pinned on a
case worked by hand; a batch over the capacity against the unsplit call; the refusals by name."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import api
from tests.classmat_checker import clear_nearest, signal_matrix
from tests.cross_checker import KEYS, bits
from tests.cross_class_checker import NA_REAL_BITS, brute_cross_class, nearest
from tests.oracle_engine import OracleEngine

NAN = float("nan")


def _quiet(call, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return call(*args, **kw)


def _data(Sq=3, Sr=5, n=40, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, Sq + Sr))
    X[rng.random((n, Sq + Sr)) < 0.08] = np.nan
    return X[:, :Sq].copy(), X[:, Sq:].copy(), [f"q{i}" for i in range(Sq)], [f"r{j}" for j in range(Sr)]


def _same(a, b, key):
    if key == "run_time":
        return
    if isinstance(a, (list, float, int)) or a is None:
        assert a == b, key
    elif np.asarray(a).dtype == object:
        assert np.array_equal(np.asarray(a), np.asarray(b)), key
    elif np.asarray(a).dtype.kind == "f":
        assert np.asarray(a).shape == np.asarray(b).shape and np.array_equal(bits(a), bits(b)), key
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), key


# ---- the checker itself ---------------------------------------------------------------------------------------------
def test_the_checker_on_a_case_worked_by_hand():
    """2 queries x 5 reference columns, classes {r0, r1}, {r2, r3, r4} and an empty third one; cor = raw / 2."""
    raw = np.array([[0.5, NAN, -0.0, 0.25, 0.75],
                    [-0.0, NAN, 0.1, 0.3, NAN]])
    cor = raw * 0.5
    med2, n_valid = brute_cross_class([cor, raw, raw, raw, raw], [0, 0, 1, 1, 1], 3)
    assert n_valid.tolist() == [[1, 3, 0], [1, 2, 0]]
    # (q0, c0): r0 alone -> 0.5.  (q0, c1): +0, 0.25, 0.75 -> the middle one.  (q0, c2): empty
    assert med2[1, 0, 0] == 0.5 and med2[0, 0, 0] == 0.25
    assert med2[1, 0, 1] == 0.25 and med2[0, 0, 1] == 0.125
    # (q1, c0): -0.0 alone -> +0 (sign bit clear) in both.  (q1, c1): 0.1 and 0.3 -> R's mean of the two
    assert bits(med2[:, 1, 0]).tolist() == [0, 0]
    assert med2[1, 1, 1] == 0.5 * (0.1 + 0.3) and med2[0, 1, 1] == 0.5 * (0.05 + 0.15)
    assert np.all(bits(med2[:, :, 2]) == NA_REAL_BITS)
    assert nearest(med2[1], n_valid, ["a", "b", "c"]) == ["a", "b"]     # 0.5 > 0.25; 0.2 > 0
    assert nearest(med2[1, :, 2:], n_valid[:, 2:], ["c"]) == [None, None]


def test_the_numpy_route_on_designed_cells():
    """api._cross_class_numpy against the checker where real data seldom goes: an empty class, a class of NA pairs
    alone, even and odd cells, zero medians of either sign, equal values."""
    rng = np.random.default_rng(3)
    raw = np.round(rng.uniform(-1, 1, size=(6, 23)), 1)          # many equal values, zeros among them
    raw[raw == 0.0] = np.where(rng.random(np.count_nonzero(raw == 0.0)) < 0.5, -0.0, 0.0)
    raw[rng.random(raw.shape) < 0.15] = NAN
    cls = rng.integers(0, 4, size=23)          # classes 0 .. 3 of 6: 4 holds NA pairs alone, 5 stays empty
    cls[[2, 9]] = 4
    raw[:, [2, 9]] = NAN
    raw[0, cls == 1] = 0.0                      # a zero median
    raw[1, cls == 1] = -0.0
    with np.errstate(invalid="ignore"):
        cor = raw / 0.8
    med2, n_valid = api._cross_class_numpy(cor, raw, cls, 6)
    want2, want_n = brute_cross_class([cor, raw, raw, raw, raw], cls, 6)
    assert np.array_equal(n_valid, want_n) and np.array_equal(bits(med2), bits(want2))
    assert np.all(n_valid[:, 4:] == 0) and np.all(bits(med2[:, :, 4:]) == NA_REAL_BITS)
    assert {int(v) & 1 for v in n_valid[n_valid > 0]} == {0, 1}
    assert bits(med2[:, :2, 1]).tolist() == [[0, 0], [0, 0]]


# ---- a PreparedReference is the plain matrix ---------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(k=4), dict(), dict(k=2, return_matrix=False, scale_max=False),
                                dict(k=3, perspective="local", alternative="greater", continuity=True)])
def test_prepared_reference_gives_the_plain_dict(kw):
    Q, R, qn, rn = _data()
    eng = OracleEngine()
    plain = _quiet(api.ici_kendalltau_cross, Q, R, query_names=qn, reference_names=rn, engine=eng, **kw)
    with api.prepare_reference(R, 8, reference_names=rn, engine=eng) as prepared:
        assert (prepared.n_feat, prepared.n_reference, prepared.query_capacity) == (40, 5, 8)
        assert prepared.reference_names == rn and prepared.class_levels is None
        got = _quiet(api.ici_kendalltau_cross, Q, prepared, query_names=qn, **kw)
        again = _quiet(api.ici_kendalltau_cross, Q[:, :2], prepared, query_names=qn[:2], **kw)
    assert list(got) == list(plain)
    for key in plain:
        _same(got[key], plain[key], key)
    assert again["query_names"] == qn[:2]
    for key in KEYS[1:]:
        if key in plain:
            assert np.array_equal(bits(again[key]), bits(np.asarray(plain[key])[:2])), key


def test_without_classes_the_plain_route_returns_todays_keys():
    Q, R, qn, rn = _data()
    res = _quiet(api.ici_kendalltau_cross, Q, R, k=2, query_names=qn, reference_names=rn, engine=OracleEngine())
    assert list(res) == list(KEYS) + ["indices", "neighbors"] + ["topk_" + k for k in KEYS] + \
        ["n_valid", "query_names", "reference_names", "max_taumax", "run_time"]


# ---- the class tables --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def signal():
    """signal_matrix() split into 30 query and 100 reference columns; reference column 5 is constant and the only member
    of its class (every pair of it is NA), reference column 6 repeats query column 3."""
    X, labels, names = signal_matrix()
    Q, R = X[:, :30].copy(), X[:, 30:].copy()
    rl = list(labels[30:])
    R[:, 5] = 1.5
    rl[5] = "solo"
    R[:, 6] = Q[:, 3]
    return Q, R, names[:30], names[30:], rl


@pytest.fixture(scope="module")
def signal_plain(signal):
    Q, R, qn, rn, _rl = signal
    return _quiet(api.ici_kendalltau_cross, Q, R, query_names=qn, reference_names=rn, engine=OracleEngine())


@pytest.mark.parametrize("scale_max", [True, False])
def test_class_tables_against_the_checker(signal, signal_plain, scale_max):
    Q, R, qn, rn, rl = signal
    res = _quiet(api.ici_kendalltau_cross, Q, R, k=3, scale_max=scale_max, query_names=qn, reference_names=rn,
                 reference_classes=rl, engine=OracleEngine())
    levels = sorted(set(rl))
    codes = [levels.index(v) for v in rl]
    assert res["class_levels"] == levels and "solo" in levels
    rect5 = [np.asarray(signal_plain[key]) for key in KEYS]
    if not scale_max:
        rect5[0] = rect5[1]
    for key in KEYS:                                        # the rectangle itself is the plain call's
        if key != "cor" or scale_max:
            assert np.array_equal(bits(res[key]), bits(signal_plain[key])), key
    want2, want_n = brute_cross_class(rect5, codes, len(levels))
    assert np.array_equal(np.asarray(res["class_n_valid"]), want_n)
    assert np.array_equal(bits(res["class_med_cor"]), bits(want2[0]))
    assert np.array_equal(bits(res["class_med_raw"]), bits(want2[1]))
    solo = levels.index("solo")
    assert np.all(want_n[:, solo] == 0) and np.all(bits(res["class_med_raw"])[:, solo] == NA_REAL_BITS)
    assert {int(v) & 1 for v in want_n[want_n > 0]} == {0, 1}          # even and odd cells
    assert np.all(want_n[17] == 0) and res["nearest_class"][17] is None    # the constant query column
    want_nearest = nearest(want2[1], want_n, levels)
    clear = clear_nearest(want2[1], want_n)
    assert clear.sum() >= 25
    assert [a for a, ok in zip(res["nearest_class"], clear) if ok] == [b for b, ok in zip(want_nearest, clear) if ok]
    assert res["nearest_class"] == want_nearest             # (the same doubles on this route: no tie to break otherwise)
    if not scale_max:
        assert np.array_equal(bits(res["class_med_cor"]), bits(res["class_med_raw"]))


def test_class_tables_are_named(signal):
    pd = pytest.importorskip("pandas")
    Q, R, qn, rn, rl = signal
    with api.prepare_reference(R, 64, reference_names=rn, reference_classes=rl, engine=OracleEngine()) as prepared:
        res = _quiet(api.ici_kendalltau_cross, Q[:, :4], prepared, return_matrix=False, query_names=qn[:4])
    assert "raw" not in res and "indices" not in res
    for key in ("class_med_cor", "class_med_raw", "class_n_valid"):
        assert isinstance(res[key], pd.DataFrame) and list(res[key].index) == qn[:4]
        assert list(res[key].columns) == res["class_levels"] == prepared.class_levels
    assert len(res["nearest_class"]) == 4


# ---- a batch over the capacity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_max", [True, False])
def test_a_batch_over_the_capacity_is_split_and_stitched(signal, scale_max):
    Q, R, qn, rn, rl = signal
    Q, qn = Q[:, :11], qn[:11]
    eng = OracleEngine()
    kw = dict(k=5, scale_max=scale_max, query_names=qn)
    with api.prepare_reference(R, 16, reference_names=rn, reference_classes=rl, engine=eng) as whole:
        one = _quiet(api.ici_kendalltau_cross, Q, whole, **kw)
    with api.prepare_reference(R, 4, reference_names=rn, reference_classes=rl, engine=eng) as narrow:
        parts = _quiet(api.ici_kendalltau_cross, Q, narrow, **kw)           # 4 + 4 + 3 columns
        firsts = [_quiet(api.ici_kendalltau_cross, Q[:, a:a + 4], narrow, k=5, query_names=qn[a:a + 4])["max_taumax"]
                  for a in (0, 4, 8)]
    assert len(set(firsts)) > 1 and max(firsts) == one["max_taumax"]       # the parts do scale differently
    assert list(parts) == list(one)
    for key in one:
        if key == "run_time":
            continue
        _same(parts[key], one[key], key)       # cor, topk_cor and class_med_cor among them: scaled again, from raw
    a, b = np.asarray(parts["class_med_cor"]), np.asarray(one["class_med_cor"])
    assert np.array_equal(bits(a), bits(b))    # even cells too: reduced again from the part's raw


def _recorded(call, *args, **kw):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        # the reference's own warnings, one per offending pair (numpy's, of the host route's divisions, are not counted)
        return call(*args, **kw), [str(x.message) for x in w if str(x.message).startswith("Warning:")]


@pytest.mark.parametrize("k", [None, 5])
def test_a_split_batch_without_its_matrix_reduces_even_cells_again(signal, k):
    """return_matrix=False, classes, scale_max and parts whose maximum is below the call's: no part kept its matrix, so
    the parts with even cells are asked for theirs once more.  class_med_cor equals the unsplit call's bits, and the
    pairs of the constant query column are warned about once, as in the unsplit call."""
    Q, R, qn, rn, rl = signal
    eng = OracleEngine()
    kw = dict(k=k, return_matrix=False, scale_max=True, query_names=qn)
    with api.prepare_reference(R, Q.shape[1], reference_names=rn, reference_classes=rl, engine=eng) as whole:
        one, warned_one = _recorded(api.ici_kendalltau_cross, Q, whole, **kw)
    asked = []
    with api.prepare_reference(R, 4, reference_names=rn, reference_classes=rl, engine=eng) as narrow:
        batch = narrow._batch
        narrow._batch = lambda *a: (asked.append(a[2]), batch(*a))[1]       # a[2]: want_matrix
        parts, warned_parts = _recorded(api.ici_kendalltau_cross, Q, narrow, **kw)
    n_parts = -(-Q.shape[1] // 4)
    assert asked[:n_parts] == [False] * n_parts and 0 < asked[n_parts:].count(True) == len(asked) - n_parts < n_parts
    assert "raw" not in parts and list(parts) == list(one)
    even = (np.asarray(one["class_n_valid"]) > 0) & ((np.asarray(one["class_n_valid"]) & 1) == 0)
    assert even.sum() >= 20
    for key in one:
        if key != "run_time":
            _same(parts[key], one[key], key)
    assert np.array_equal(bits(np.asarray(parts["class_med_cor"])), bits(np.asarray(one["class_med_cor"])))
    assert len(warned_one) > 0 and sorted(warned_parts) == sorted(warned_one)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    Q, R, qn, rn = _data()
    eng = OracleEngine()
    with pytest.raises(ValueError, match="`query_capacity` must be an integer in 1 .. 65535"):
        api.prepare_reference(R, 0, reference_names=rn, engine=eng)
    with pytest.raises(ValueError, match="Colnames of `reference`"):
        api.prepare_reference(R, 4, engine=eng)
    with pytest.raises(ValueError, match="`reference_classes` must give one class per column"):
        api.prepare_reference(R, 4, reference_names=rn, reference_classes=["a", "b"], engine=eng)
    prepared = api.prepare_reference(R, 4, global_na=(NAN, 0), reference_names=rn, engine=eng)
    with pytest.raises(ValueError, match="`global_na` differs"):
        api.ici_kendalltau_cross(Q, prepared, global_na=(NAN, float("inf"), 0), query_names=qn)
    with pytest.raises(ValueError, match="`query` has 39 rows .* `reference` has 40"):
        api.ici_kendalltau_cross(Q[:39], prepared, query_names=qn)
    with pytest.raises(ValueError, match="`reference_names` and `reference_classes` belong to the PreparedReference"):
        api.ici_kendalltau_cross(Q, prepared, query_names=qn, reference_names=rn)
    with pytest.raises(ValueError, match="nothing to return"):
        api.ici_kendalltau_cross(Q, prepared, return_matrix=False, query_names=qn)
    # the same rule in another order, or left at the default, is no conflict
    a = _quiet(api.ici_kendalltau_cross, Q, prepared, global_na=(0, NAN, NAN), query_names=qn)
    b = _quiet(api.ici_kendalltau_cross, Q, prepared, query_names=qn)
    want = _quiet(api.ici_kendalltau_cross, Q, R, global_na=(NAN, 0), query_names=qn, reference_names=rn, engine=eng)
    for key in KEYS:
        assert np.array_equal(bits(a[key]), bits(want[key])) and np.array_equal(bits(b[key]), bits(want[key])), key
    prepared.close()
    with pytest.raises(ValueError, match="has been closed"):
        api.ici_kendalltau_cross(Q, prepared, query_names=qn)


def test_empty_query_against_a_prepared_reference():
    Q, R, qn, rn = _data()
    with api.prepare_reference(R, 4, reference_names=rn, reference_classes=list("aabbc"), engine=OracleEngine()) as p:
        res = _quiet(api.ici_kendalltau_cross, Q[:, :0], p, k=2, query_names=[])
    assert np.asarray(res["raw"]).shape == (0, 5) and res["indices"].shape == (0, 2)
    assert np.asarray(res["class_med_raw"]).shape == (0, 3) and res["nearest_class"] == []
    assert res["max_taumax"] == -np.inf
