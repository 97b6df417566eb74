"""icikt_class_medians_f64 / _in / _csc on the GPU: every sample's median ICI-Kendall-tau within its class, reduced on
the device.

The reference is the brute-force checker (tests/medians_checker.py) applied to Context.matrix called with the
within-class pair list: med2 must be BITWISE equal (a sample without partners carries R's NA_real_ bits), n_valid,
reason_counts and max_taumax equal.  The shapes are the smallest that reach each part of the kernels: both parities of
the partner count, one and several 256-wide passes, staged and re-read keys, runs of equal values around the middle,
blocks of one row and slices that end mid-class."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.medians_checker import NA_REAL_BITS, bits, brute_medians, class_pairs
from tests.test_gpu_topk import _edge_matrix

pytestmark = pytest.mark.gpu

_REF = {}   # (data key, perspective, scale_max) -> (med2, n_valid, max_taumax, reason_counts): computed once


def _continuous(S, n, seed=11):
    rng = np.random.default_rng(seed + 1000 * S + n)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X


def _interleaved(S=130):
    """classes of 1, 2, 3, 60 and 64 samples in shuffled order; class index 2 of the 6 stays empty"""
    cls = np.repeat([0, 1, 3, 4, 5], [1, 2, 3, 60, 64]).astype(np.int32)
    assert cls.shape[0] == S
    np.random.default_rng(4).shuffle(cls)
    return cls, 6


def _five_classes(S):
    return np.random.default_rng(9).integers(0, 5, S).astype(np.int32), 5


def _reference(ctx, key, X, cls, n_class, global_na=None, perspective="global", scale_max=True):
    rk = (key, perspective, scale_max)
    if rk not in _REF:
        S = X.shape[1]
        pi, pj = class_pairs(np.zeros(S, dtype=np.int32) if cls is None else cls, 1 if cls is None else n_class)
        out5, _keep, rc5 = ctx.matrix(X, global_na, pi, pj, perspective, "two.sided", False, 0, scale_max, True,
                                      want_keep=False)
        med2, n_valid = brute_medians(out5, cls)
        tm = out5[3][pi, pj]
        tm = tm[~np.isnan(tm)]
        _REF[rk] = (med2, n_valid, float(tm.max()) if tm.size else -np.inf, rc5, out5)
    return _REF[rk]


def _assert_same(got, ref):
    med2, n_valid, mx, rc5 = got
    print("n_valid", n_valid.min(), n_valid.max(), "max_taumax", mx, ref[2], "differing cells",
          int(np.sum(bits(med2) != bits(ref[0]))))
    assert np.array_equal(n_valid, ref[1])
    assert np.array_equal(bits(med2), bits(ref[0]))
    assert np.all((bits(med2) == NA_REAL_BITS) == (n_valid == 0)[None, :])
    assert mx == ref[2]
    assert np.array_equal(rc5, ref[3])


@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("S", [2, 3, 65, 130])
def test_small_shapes_one_class(hip_ctx, S, n):
    X = _continuous(S, n)
    ref = _reference(hip_ctx, ("cont", S, n, "one"), X, None, 1)
    _assert_same(hip_ctx.class_medians(X), ref)
    assert np.all(ref[1] == S - 1)
    # an explicit class index per sample says the same as none at all
    _assert_same(hip_ctx.class_medians(X, np.zeros(S, dtype=np.int32), 1), ref)


@pytest.mark.parametrize("cfg", [("global", True), ("global", False), ("local", True)])
def test_interleaved_classes(hip_ctx, cfg):
    perspective, scale_max = cfg
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _interleaved(S)
    ref = _reference(hip_ctx, ("cont", S, n, "inter"), X, cls, n_class, None, perspective, scale_max)
    got = hip_ctx.class_medians(X, cls, n_class, None, perspective, "two.sided", False, 0, scale_max)
    _assert_same(got, ref)
    sizes = np.bincount(cls, minlength=n_class)[cls]
    assert np.array_equal(got[1], sizes - 1) and 0 in got[1]           # (continuous data: every pair is valid)
    if not scale_max:
        assert np.array_equal(bits(got[0][0]), bits(got[0][1]))
    else:   # the scale is the within-class maximum
        whole = _reference(hip_ctx, ("cont", S, n, "one"), X, None, 1)
        assert got[2] <= whole[2]


def test_na_pairs(plan_ctx):
    """constant, all-missing and single-row columns: pairs of reasons 1-4.  Classes {7, 10}: NA partners alone;
    {3, 0, 1}: the constant column 3 has none, 0 and 1 exactly one; {2, 5, 8}: exactly two each."""
    X = _edge_matrix()
    S = X.shape[1]
    cls = np.array([1, 1, 2, 1, 3, 2, 3, 0, 2, 3, 0, 3], dtype=np.int32)
    ref = _reference(plan_ctx, ("edge", "classes"), X, cls, 4)
    assert ref[1].tolist() == [1, 1, 2, 0, 3, 2, 3, 0, 2, 3, 0, 3]
    assert ref[3][1:].sum() > 0
    for spec in (None, "tkblock=3", "medlds=1"):
        plan_ctx.debug_set_plan(spec)
        _assert_same(plan_ctx.class_medians(X, cls, 4), ref)
    # one class: every reason code among a sample's pairs
    ref1 = _reference(plan_ctx, ("edge", "one"), X, None, 1)
    assert ref1[1][3] == 0 and ref1[1][7] == 0 and ref1[3][1:].sum() >= S - 1
    for spec in (None, "tkblock=1", "medlds=4"):
        plan_ctx.debug_set_plan(spec)
        _assert_same(plan_ctx.class_medians(X), ref1)


@pytest.mark.parametrize("S", [1500, 1501])
def test_equal_values_at_the_median(hip_ctx, S):
    """16 rows give tau a few hundred distinct values at most among 1 499 / 1 500 partners, exact zeros among them: the
    middle of a sample's keys lies inside a run of equal ones, or at its edge."""
    X = _continuous(S, 16)
    ref = _reference(hip_ctx, ("cont", S, 16, "one"), X, None, 1)
    raw_row = ref[4][1][0][1:]
    assert len(np.unique(raw_row[~np.isnan(raw_row)])) < 1000 and np.any(ref[4][1] == 0.0)
    _assert_same(hip_ctx.class_medians(X), ref)


def test_equal_values_with_five_classes(hip_ctx):
    S = 1500
    X = _continuous(S, 16)
    cls, n_class = _five_classes(S)
    ref = _reference(hip_ctx, ("cont", S, 16, "five"), X, cls, n_class)
    _assert_same(hip_ctx.class_medians(X, cls, n_class), ref)


@pytest.mark.parametrize("case", ["130-one", "130-interleaved", "1500-one", "1500-five"])
def test_both_select_paths(plan_ctx, case):
    """medlds=64: samples with more than 64 partners re-read the kept plane in every pass (the classes of 60 and 64
    samples still stage their 59 / 63 keys: medlds=0 makes them re-read as well)"""
    S = int(case.split("-")[0])
    n = 40 if S == 130 else 16
    X = _continuous(S, n)
    kind = case.split("-")[1]
    cls, n_class = {"one": (None, 1), "interleaved": _interleaved(), "five": _five_classes(S)}[kind]
    ref = _reference(plan_ctx, ("cont", S, n, {"interleaved": "inter"}.get(kind, kind)), X, cls, n_class)
    outs = []
    for spec in (None, "medlds=64", "medlds=0"):
        plan_ctx.debug_set_plan(spec)
        outs.append(plan_ctx.class_medians(X, cls, n_class))
        _assert_same(outs[-1], ref)
    for got in outs[1:]:
        assert np.array_equal(bits(got[0]), bits(outs[0][0])) and np.array_equal(got[1], outs[0][1])


def test_block_cuts_give_identical_output(plan_ctx):
    S, n = 130, 40
    X = _continuous(S, n)
    ref = _reference(plan_ctx, ("cont", S, n, "one"), X, None, 1)
    for spec in ("tkblock=1", "tkblock=1000", None):
        plan_ctx.debug_set_plan(spec)
        _assert_same(plan_ctx.class_medians(X), ref)
    cls, n_class = _interleaved(S)
    ref = _reference(plan_ctx, ("cont", S, n, "inter"), X, cls, n_class)
    for spec in ("tkblock=1000", None):
        plan_ctx.debug_set_plan(spec)
        _assert_same(plan_ctx.class_medians(X, cls, n_class), ref)


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.class_medians(X64, *args)
    finally:
        ctx.f64_entries = False


def test_float32_row_major_view_matches_float64(hip_ctx):
    S, n = 65, 40
    rng = np.random.default_rng(21)
    X32 = np.ascontiguousarray(rng.standard_normal((n, S)).astype(np.float32))
    X32[rng.random((n, S)) < 0.08] = np.nan
    assert X32.flags.c_contiguous and _lib.input_view(X32)[2] == _lib.ORDER_ROW
    X64 = np.asfortranarray(X32, dtype=np.float64)
    cls = (np.arange(S) % 3).astype(np.int32)
    want = _f64_entry(hip_ctx, X64, cls, 3)
    got = hip_ctx.class_medians(X32, cls, 3)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    assert got[2] == want[2] and np.array_equal(got[3], want[3])
    _assert_same(got, _reference(hip_ctx, "f32", X64, cls, 3))


def test_scipy_csc_matches_dense(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    gna = [np.nan, np.inf, 0.0]
    cls = (np.arange(S) % 3).astype(np.int32)
    want = _f64_entry(hip_ctx, X, cls, 3, gna)
    got = hip_ctx.class_medians(A, cls, 3, gna)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    assert got[2] == want[2] and np.array_equal(got[3], want[3])
    _assert_same(got, _reference(hip_ctx, "csc", X, cls, 3, gna))


def test_refusals_leave_outputs_and_context_untouched(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.pairs(X)                                   # a prepared matrix and a pair list to keep
    L = _lib.lib()
    E_INVALID = -1
    big = np.zeros((1, 65536), order="F")
    ok_cls = np.zeros(S, dtype=np.int32)

    def call(Xa, n_feat, n_samp, cls, n_class, perspective, null_med2=False):
        med2 = np.full((2, n_samp), 123.25)
        n_valid = np.full(n_samp, -7, dtype=np.int32)
        mx = np.full(1, 55.5)
        rc5 = np.full(5, -9, dtype=np.int64)
        rc = L.icikt_class_medians_f64(hip_ctx._h, _lib._ptr(Xa), n_feat, n_samp, max(n_feat, 1), None, 0, _lib._ptr(cls),
                                       n_class, perspective, 0, 0, 0, 1, None if null_med2 else _lib._ptr(med2),
                                       _lib._ptr(n_valid), _lib._ptr(mx), _lib._ptr(rc5))
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == E_INVALID, rc
        assert msg and b"class_medians" in msg, msg
        assert np.all(med2 == 123.25) and np.all(n_valid == -7) and mx[0] == 55.5 and np.all(rc5 == -9)
        assert hip_ctx.num_pairs() == S * (S - 1) // 2    # the refused call touched nothing
        return msg.decode()

    bad = ok_cls.copy()
    bad[5] = 2
    assert "cls[5] = 2" in call(X, n, S, bad, 2, 1)
    bad[5] = -1
    assert "cls[5] = -1" in call(X, n, S, bad, 2, 1)
    assert "ICIKT_TOPK_MAX_SAMPLES" in call(big, 1, 65536, np.zeros(65536, dtype=np.int32), 1, 1)
    assert "null output (med2)" in call(X, n, S, ok_cls, 1, 1, null_med2=True)
    assert "perspective" in call(X, n, S, ok_cls, 1, 7)
    with pytest.raises(_lib.IciktError, match="class_medians: perspective"):
        hip_ctx.class_medians(X, perspective="sideways")
    out, _cnt, rsn = hip_ctx.pairs(X)                  # and the next ordinary call succeeds
    assert out.shape == (S * (S - 1) // 2, 4) and np.all(rsn == 0)


def test_state_after_a_successful_call(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    for cls in (None, (np.arange(S) % 2).astype(np.int32), np.arange(S, dtype=np.int32)):
        hip_ctx.pairs(X)
        med2, n_valid, mx, rc5 = hip_ctx.class_medians(X, cls, S)
        assert hip_ctx.num_pairs() == -1
        rc = _lib.lib().icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
        assert rc == -5, rc                            # ICIKT_E_STATE: nothing prepared
    # (the last call: singletons alone -- no pair computed, every median NA, the scale -Inf)
    assert np.all(n_valid == 0) and np.all(bits(med2) == NA_REAL_BITS) and mx == -np.inf and rc5.sum() == 0
    out, _cnt, _rsn = hip_ctx.pairs(X)
    assert out.shape[0] == S * (S - 1) // 2


def test_front_end_matches_the_checker_engine(hip_ctx):
    """The HIP engine and the CPU oracle agree to 1e-10 on a pair's values, not bitwise (smoke() asserts that bound); a
    median is one of a sample's values or the mean of two, so it moves by no more than they do.  Everything that is
    not a float -- names, labels, partner counts, the NA pattern, the warnings -- is equal."""
    from tests.oracle_engine import OracleEngine
    S, n = 130, 40
    X = _continuous(S, n).copy()
    X[:, 17] = 1.5                                     # a constant column: a warning per pair of its class
    cls, _n_class = _interleaved(S)
    labels = [f"batch{k}" for k in cls]
    names = [f"s{i}" for i in range(S)]
    res, msgs = [], []
    for eng in (api.HipEngine(), OracleEngine()):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            res.append(api.ici_kendalltau_medians(X, sample_classes=labels, colnames=names, engine=eng))
        msgs.append(sorted(str(x.message) for x in w if str(x.message) in _lib.REASON_WARNINGS.values()))
    got, want = res
    assert msgs[0] == msgs[1] and len(msgs[0]) == np.sum(cls == cls[17]) - 1
    assert got["sample_id"] == want["sample_id"] == names
    assert got["sample_class"] == want["sample_class"] == labels
    assert np.array_equal(got["n_valid"], want["n_valid"]) and got["n_valid"][17] == 0
    for key in ("med_cor", "med_raw"):
        both = ~np.isnan(got[key]) & ~np.isnan(want[key])
        print(key, np.max(np.abs(got[key][both] - want[key][both])))
        assert np.array_equal(bits(got[key]) == NA_REAL_BITS, bits(want[key]) == NA_REAL_BITS)
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key]))
        assert np.allclose(got[key], want[key], rtol=0, atol=1e-10, equal_nan=True), key
    assert abs(got["max_taumax"] - want["max_taumax"]) <= 1e-10
