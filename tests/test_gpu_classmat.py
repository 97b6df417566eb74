"""icikt_class_matrix_f64 / _in / _csc on the GPU: every sample's median ICI-Kendall-tau to every class, reduced on the
device.

The reference is the brute-force checker (tests/classmat_checker.py) applied to Context.matrix over all pairs, computed
once per data set: med2 must be BITWISE equal (a cell without partners carries R's NA_real_ bits), n_valid,
reason_counts and max_taumax equal.  The shapes are the smallest that reach each part of the kernel: both parities of
a cell's partner count, cells of one key, cells with and without the sample itself, empty classes, one and several
256-wide passes, staged and re-read keys, runs of equal values around the middle, blocks of one row."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.classmat_checker import NA_REAL_BITS, bits, brute_class_matrix, clear_nearest, signal_matrix
from tests.test_gpu_medians import _continuous, _five_classes, _interleaved
from tests.test_gpu_topk import _edge_matrix

pytestmark = pytest.mark.gpu

_FULL = {}  # (data key, perspective, scale_max) -> (out5, max_taumax, reason_counts) of Context.matrix: computed once
_REF = {}   # (data key, layout key, perspective, scale_max) -> (med2, n_valid, max_taumax, reason_counts)


def _reference(ctx, key, layout, X, cls, n_class, global_na=None, perspective="global", scale_max=True):
    fk = (key, perspective, scale_max)
    if fk not in _FULL:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, perspective, "two.sided", False, 0, scale_max, True,
                                      want_keep=False)
        tm = out5[3][np.triu_indices(X.shape[1], k=1)]
        tm = tm[~np.isnan(tm)]
        _FULL[fk] = (out5, float(tm.max()) if tm.size else -np.inf, rc5)
    rk = (key, layout, perspective, scale_max)
    if rk not in _REF:
        out5, mx, rc5 = _FULL[fk]
        med2, n_valid = brute_class_matrix(out5, cls, 1 if cls is None else n_class)
        _REF[rk] = (med2, n_valid, mx, rc5)
    return _REF[rk]


def _assert_same(got, ref):
    med2, n_valid, mx, rc5 = got
    print("shape", med2.shape, "n_valid", n_valid.min(), n_valid.max(), "max_taumax", mx, ref[2], "differing cells",
          int(np.sum(bits(med2) != bits(ref[0]))) if med2.shape == ref[0].shape else "shape")
    assert med2.shape == ref[0].shape and n_valid.shape == ref[1].shape
    assert np.array_equal(n_valid, ref[1])
    assert np.array_equal(bits(med2), bits(ref[0]))
    assert np.all((bits(med2) == NA_REAL_BITS) == (n_valid == 0)[None, :, :])
    assert mx == ref[2]
    assert np.array_equal(rc5, ref[3])


def _same_bits(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
            and np.array_equal(a[3], b[3]))


@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("S", [2, 3, 65, 130])
def test_small_shapes_one_class(hip_ctx, S, n):
    X = _continuous(S, n)
    ref = _reference(hip_ctx, ("cont", S, n), "one", X, None, 1)
    got = hip_ctx.class_matrix(X)
    assert got[0].shape == (2, S, 1) and got[1].shape == (S, 1)
    _assert_same(got, ref)
    assert np.all(ref[1] == S - 1)
    # an explicit class index per sample says the same as none at all
    _assert_same(hip_ctx.class_matrix(X, np.zeros(S, dtype=np.int32), 1), ref)


@pytest.mark.parametrize("cfg", [("global", True), ("global", False), ("local", True)])
def test_interleaved_classes(hip_ctx, cfg):
    perspective, scale_max = cfg
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _interleaved(S)
    ref = _reference(hip_ctx, ("cont", S, n), "inter", X, cls, n_class, None, perspective, scale_max)
    got = hip_ctx.class_matrix(X, cls, n_class, None, perspective, "two.sided", False, 0, scale_max)
    _assert_same(got, ref)
    # continuous data, every pair valid: a cell has the class's size, less one in the sample's own column
    sizes = np.bincount(cls, minlength=n_class)
    want_n = np.tile(sizes, (S, 1))
    want_n[np.arange(S), cls] -= 1
    assert np.array_equal(got[1], want_n)
    counts = set(got[1].ravel().tolist())
    assert {0, 1, 2, 3, 59, 60, 63, 64} <= counts        # both parities, T = 1, the empty class, the singleton's own cell
    if not scale_max:
        assert np.array_equal(bits(got[0][0]), bits(got[0][1]))


def test_na_pairs(plan_ctx):
    """constant, all-missing and single-row columns: pairs with a reason code.  The constant column 3 and the all-missing
    column 7 have NA partners alone in every cell of their rows; class 0 = {7, 10} gives sample 10 the partner 7 alone
    and every other sample the one partner 10; class 1 = {0, 1, 3} holds a member that is no one's partner."""
    X = _edge_matrix()
    S = X.shape[1]
    cls = np.array([1, 1, 2, 1, 3, 2, 3, 0, 2, 3, 0, 3], dtype=np.int32)
    ref = _reference(plan_ctx, "edge", "classes", X, cls, 4)
    assert np.all(ref[1][[3, 7], :] == 0) and ref[1][10, 0] == 0 and ref[1].max() >= 3
    assert ref[1][:, 0].tolist() == [1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1] and ref[1][0, 1] == 1 and ref[1][2, 1] == 2
    assert ref[3][1:].sum() > 0
    for spec in (None, "tkblock=3", "medlds=1"):
        plan_ctx.debug_set_plan(spec)
        _assert_same(plan_ctx.class_matrix(X, cls, 4), ref)
    # one class: every reason code among a sample's pairs
    ref1 = _reference(plan_ctx, "edge", "one", X, None, 1)
    assert ref1[1][3, 0] == 0 and ref1[1][7, 0] == 0 and ref1[3][1:].sum() >= S - 1
    for spec in (None, "tkblock=1", "medlds=4"):
        plan_ctx.debug_set_plan(spec)
        _assert_same(plan_ctx.class_matrix(X), ref1)


@pytest.mark.parametrize("S", [1500, 1501])
def test_equal_values_at_the_median(hip_ctx, S):
    """16 rows give tau a few hundred distinct values at most among 1 499 / 1 500 partners, exact zeros among them: the
    middle of a cell's keys lies inside a run of equal ones, or at its edge; six 256-wide passes per digit."""
    X = _continuous(S, 16)
    ref = _reference(hip_ctx, ("cont", S, 16), "one", X, None, 1)
    out5 = _FULL[(("cont", S, 16), "global", True)][0]
    raw_row = out5[1][0][1:]
    assert len(np.unique(raw_row[~np.isnan(raw_row)])) < 1000 and np.any(out5[1] == 0.0)
    _assert_same(hip_ctx.class_matrix(X), ref)


@pytest.mark.parametrize("S", [1500, 1501])
def test_equal_values_with_five_classes(hip_ctx, S):
    X = _continuous(S, 16)
    cls, n_class = _five_classes(S)
    assert np.bincount(cls, minlength=5).min() > 256       # about 300 each: two passes of 256 per cell
    ref = _reference(hip_ctx, ("cont", S, 16), "five", X, cls, n_class)
    _assert_same(hip_ctx.class_matrix(X, cls, n_class), ref)


@pytest.mark.parametrize("case", ["130-one", "130-interleaved", "1500-five"])
def test_block_cuts_and_both_select_paths(plan_ctx, case):
    """tkblock=1: a row per block; tkblock=1000: several rows; medlds=64: cells of more than 64 keys re-read the kept
    plane in every pass (the classes of 60 and 64 samples still stage their keys: medlds=0 makes them re-read too)"""
    S = int(case.split("-")[0])
    n = 40 if S == 130 else 16
    X = _continuous(S, n)
    kind = case.split("-")[1]
    cls, n_class = {"one": (None, 1), "interleaved": _interleaved(), "five": _five_classes(S)}[kind]
    ref = _reference(plan_ctx, ("cont", S, n), {"interleaved": "inter"}.get(kind, kind), X, cls, n_class)
    cuts = ("tkblock=1", "tkblock=1000") if S == 130 else ("tkblock=200000",)
    outs = []
    for spec in (None,) + cuts + ("medlds=0", "medlds=64"):
        plan_ctx.debug_set_plan(spec)
        outs.append(plan_ctx.class_matrix(X, cls, n_class))
        _assert_same(outs[-1], ref)
    for got in outs[1:]:
        assert _same_bits(got, outs[0])


@pytest.mark.parametrize("kind", ["interleaved", "one"])
def test_identities_with_class_medians(hip_ctx, kind):
    """The own-class column carries class_medians' med_raw and n_valid bit for bit; with one class med_cor agrees too
    (both entries then scale by the same maximum)."""
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _interleaved(S) if kind == "interleaved" else (np.zeros(S, dtype=np.int32), 1)
    med2, n_valid, mx, rc5 = hip_ctx.class_matrix(X, cls, n_class)
    own2, own_n, own_mx, _rc = hip_ctx.class_medians(X, cls, n_class)
    rows = np.arange(S)
    assert np.array_equal(bits(med2[1][rows, cls]), bits(own2[1]))
    assert np.array_equal(n_valid[rows, cls], own_n)
    assert 0 in own_n or kind == "one"
    if kind == "one":
        assert np.array_equal(bits(med2[0][:, 0]), bits(own2[0])) and mx == own_mx
        assert rc5.sum() == S * (S - 1) // 2
    else:
        assert own_mx <= mx                                # the within-class maximum against the one over all pairs


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.class_matrix(X64, *args)
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
    got = hip_ctx.class_matrix(X32, cls, 3)
    assert _same_bits(got, want)
    _assert_same(got, _reference(hip_ctx, "f32", "mod3", X64, cls, 3))


def test_scipy_csc_matches_dense(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    gna = [np.nan, np.inf, 0.0]
    cls = (np.arange(S) % 3).astype(np.int32)
    want = _f64_entry(hip_ctx, X, cls, 3, gna)
    got = hip_ctx.class_matrix(A, cls, 3, gna)
    assert _same_bits(got, want)
    _assert_same(got, _reference(hip_ctx, "csc", "mod3", X, cls, 3, gna))


def test_refusals_leave_outputs_and_context_untouched(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.pairs(X)                                   # a prepared matrix and a pair list to keep
    L = _lib.lib()
    E_INVALID = -1
    big = np.zeros((1, 65536), order="F")
    ok_cls = np.zeros(S, dtype=np.int32)

    def call(Xa, n_feat, n_samp, cls, n_class, perspective, null_med2=False):
        room = n_class if 1 <= n_class <= 4 else 1     # (a refused call writes nothing: no room for what it cannot fill)
        med2 = np.full((2, room, n_samp), 123.25)
        n_valid = np.full((room, n_samp), -7, dtype=np.int32)
        mx = np.full(1, 55.5)
        rc5 = np.full(5, -9, dtype=np.int64)
        rc = L.icikt_class_matrix_f64(hip_ctx._h, _lib._ptr(Xa), n_feat, n_samp, max(n_feat, 1), None, 0, _lib._ptr(cls),
                                      n_class, perspective, 0, 0, 0, 1, None if null_med2 else _lib._ptr(med2),
                                      _lib._ptr(n_valid), _lib._ptr(mx), _lib._ptr(rc5))
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == E_INVALID, rc
        assert msg and msg.startswith(b"class_matrix:"), msg
        assert np.all(med2 == 123.25) and np.all(n_valid == -7) and mx[0] == 55.5 and np.all(rc5 == -9)
        assert hip_ctx.num_pairs() == S * (S - 1) // 2    # the refused call touched nothing
        return msg.decode()

    bad = ok_cls.copy()
    bad[5] = 2
    assert "cls[5] = 2" in call(X, n, S, bad, 2, 1)
    bad[5] = -1
    assert "cls[5] = -1" in call(X, n, S, bad, 2, 1)
    msg = call(X, n, S, ok_cls, 65536, 1)
    assert "n_class exceeds 65535" in msg and "grid" in msg
    assert "n_class must be at least 1" in call(X, n, S, ok_cls, 0, 1)
    assert "ICIKT_TOPK_MAX_SAMPLES" in call(big, 1, 65536, np.zeros(65536, dtype=np.int32), 1, 1)
    assert "null output (med2)" in call(X, n, S, ok_cls, 1, 1, null_med2=True)
    assert "perspective" in call(X, n, S, ok_cls, 1, 7)
    with pytest.raises(_lib.IciktError, match="class_matrix: perspective"):
        hip_ctx.class_matrix(X, perspective="sideways")
    with pytest.raises(_lib.IciktError, match="class_matrix: n_class exceeds 65535"):
        hip_ctx.class_matrix(X, ok_cls, 65536)
    assert hip_ctx.num_pairs() == S * (S - 1) // 2
    out, _cnt, rsn = hip_ctx.pairs(X)                  # and the next ordinary call succeeds
    assert out.shape == (S * (S - 1) // 2, 4) and np.all(rsn == 0)


def test_state_after_a_successful_call(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    for cls in (None, (np.arange(S) % 2).astype(np.int32), np.arange(S, dtype=np.int32)):
        hip_ctx.pairs(X)
        med2, n_valid, mx, rc5 = hip_ctx.class_matrix(X, cls, S)
        assert hip_ctx.num_pairs() == -1
        rc = _lib.lib().icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
        assert rc == -5, rc                            # ICIKT_E_STATE: nothing prepared
    # (the last call: singletons alone -- every own cell NA, every other cell one key; all pairs were computed)
    own = np.eye(S, dtype=bool)
    assert med2.shape == (2, S, S) and np.array_equal(n_valid, (~own).astype(np.int32))
    assert np.array_equal(bits(med2[1]) == NA_REAL_BITS, own) and np.isfinite(mx) and rc5[0] == S * (S - 1) // 2
    out, _cnt, _rsn = hip_ctx.pairs(X)
    assert out.shape[0] == S * (S - 1) // 2
    assert np.array_equal(bits(med2[1][~own]), bits(np.where(out[:, 0] == 0.0, 0.0, out[:, 0])[_sym_index(S)][~own]))


def _sym_index(S):
    """[S, S]: the combn index of the pair (min, max) of every off-diagonal cell (0 on the diagonal)"""
    idx = np.zeros((S, S), dtype=np.int64)
    iu = np.triu_indices(S, k=1)
    idx[iu] = np.arange(len(iu[0]))
    return idx + idx.T


def test_front_end_matches_the_checker_engine(hip_ctx):
    """The HIP engine and the CPU oracle agree to 1e-10 on a pair's values, not bitwise (smoke() asserts that bound); a
    median is one of a cell's values or the mean of two, so it moves by no more than they do.  Everything that is not a
    float -- names, labels, levels, partner counts, the NA pattern, the warnings -- is equal; nearest_class is compared
    where the oracle's two best cells are more than 1e-9 apart (tests/test_classmat_host.py asserts that share)."""
    from tests.oracle_engine import OracleEngine
    X, labels, names = signal_matrix()
    S = len(names)
    res, msgs = [], []
    for eng in (api.HipEngine(), OracleEngine()):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            res.append(api.ici_kendalltau_class_matrix(X, labels, colnames=names, engine=eng))
        msgs.append(sorted(str(x.message) for x in w if str(x.message) in _lib.REASON_WARNINGS.values()))
    got, want = res
    assert msgs[0] == msgs[1] and len(msgs[0]) == S - 1            # the constant column's pairs
    assert got["sample_id"] == want["sample_id"] == names
    assert got["sample_class"] == want["sample_class"] == labels
    assert got["classes"] == want["classes"] == sorted(set(labels))
    assert np.array_equal(got["n_valid"], want["n_valid"]) and np.all(got["n_valid"][17] == 0)
    for key in ("med_cor", "med_raw"):
        assert got[key].shape == want[key].shape == (S, len(got["classes"]))
        both = ~np.isnan(got[key]) & ~np.isnan(want[key])
        print(key, np.max(np.abs(got[key][both] - want[key][both])))
        assert np.array_equal(bits(got[key]) == NA_REAL_BITS, bits(want[key]) == NA_REAL_BITS)
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key]))
        assert np.allclose(got[key], want[key], rtol=0, atol=1e-10, equal_nan=True), key
    assert abs(got["max_taumax"] - want["max_taumax"]) <= 1e-10
    clear = clear_nearest(want["med_raw"], want["n_valid"])
    print("clear", int(clear.sum()), "of", S)
    assert clear.mean() >= 0.9
    assert [v for v, ok in zip(got["nearest_class"], clear) if ok] == [v for v, ok in zip(want["nearest_class"], clear) if ok]
    assert got["nearest_class"][17] is None and want["nearest_class"][17] is None
