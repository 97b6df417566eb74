"""icikt_quantiles_f64 / _in / _csc on the GPU: exact quantiles and a histogram of raw over all pairs, split into all /
within-class / between-class pairs, reduced on the device.

The reference is the brute-force checker (tests/quantiles_checker.py) applied to Context.matrix on the same input:
order2 and q2 must be BITWISE equal (a group without a value carries R's NA_real_ bits), n_valid, n_na, hist, outside,
reason_counts and max_taumax equal.  The shapes are the smallest that reach each part of the kernels: fewer pairs than
one workgroup and several workgroups, ranks inside runs of equal keys, all-NA groups, blocks of one row and blocks that
end mid-triangle, one target per select batch and several."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.quantiles_checker import NA_REAL_BITS, PROBS, bits, brute_quantiles
from tests.test_gpu_medians import _continuous, _five_classes, _interleaved
from tests.test_gpu_topk import _edge_matrix

pytestmark = pytest.mark.gpu

BREAKS7 = np.linspace(-1.0, 1.0, 8)
BREAKS200 = np.linspace(-1.0, 1.0, 201)
_OUT5 = {}   # (data key, perspective, scale_max) -> (out5, max_taumax, reason_counts): computed once
_REF = {}    # (... , class key, probs, breaks key) -> the checker's answer


def _few_rows(S=1500, n=16):
    """16 rows with 2 % missing cells: over all pairs tau takes a few hundred distinct values (the medians tests'
    _continuous, with 8 %, gives 1 667 at this shape)"""
    rng = np.random.default_rng(16)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.02] = np.nan
    return X


def _matrices(ctx, key, X, global_na=None, perspective="global", scale_max=True):
    mk = (key, perspective, scale_max)
    if mk not in _OUT5:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, perspective, "two.sided", False, 0, scale_max, True,
                                      want_keep=False)
        iu, ju = np.triu_indices(X.shape[1], k=1)
        tm = out5[3][iu, ju]
        tm = tm[~np.isnan(tm)]
        _OUT5[mk] = (out5, float(tm.max()) if tm.size else -np.inf, rc5)
    return _OUT5[mk]


def _reference(ctx, key, X, cls, cls_key, probs=PROBS, breaks=BREAKS7, **kw):
    out5, mx, rc5 = _matrices(ctx, key, X, **kw)
    rk = (key, kw.get("perspective", "global"), kw.get("scale_max", True), cls_key, tuple(probs),
          None if breaks is None else tuple(breaks))
    if rk not in _REF:
        _REF[rk] = brute_quantiles(out5, cls, probs, breaks) + (mx, rc5)
    return _REF[rk]


def _assert_same(got, ref):
    q2, order2, n_valid, n_na, hist, outside, mx, rc5 = got
    print("n_valid", n_valid, "n_na", n_na, "max_taumax", mx, ref[6], "differing cells",
          int(np.sum(bits(q2) != bits(ref[0]))), int(np.sum(bits(order2) != bits(ref[1]))))
    assert np.array_equal(n_valid, ref[2]) and np.array_equal(n_na, ref[3])
    assert np.array_equal(hist, ref[4]) and np.array_equal(outside, ref[5])
    assert np.array_equal(bits(order2), bits(ref[1]))
    assert np.array_equal(bits(q2), bits(ref[0]))
    assert np.all((bits(q2) == NA_REAL_BITS) == (n_valid == 0)[None, :, None])
    assert mx == ref[6]
    assert np.array_equal(rc5, ref[7])


def _same_bits(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray) and x.dtype == np.float64:
            assert np.array_equal(bits(x), bits(y))
        else:
            assert np.array_equal(x, y)


@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("S", [2, 3, 65, 130])
def test_small_and_mid_shapes(hip_ctx, S, n):
    """1, 3, 2 080 and 8 385 pairs, with one group and with classes.  The interleaved classes of 1/2/3/60/64 samples
    partition 130 samples and nothing else, so they run at S = 130; S = 2, 3 and 65 take two alternating classes, which
    at S = 2 leave the within-class group empty."""
    X = _continuous(S, n)
    for breaks, bk in ((BREAKS7, 7), (BREAKS200, 200)):
        ref = _reference(hip_ctx, ("cont", S, n), X, None, "one", breaks=breaks)
        got = hip_ctx.quantiles(X, PROBS, breaks)
        _assert_same(got, ref)
        assert got[2][0] == S * (S - 1) // 2 and got[4].sum() == got[2][0]
    # classes: the interleaved 1/2/3/60/64 at S = 130, else two alternating classes (S = 2: no within-class pair)
    cls, n_class = _interleaved(S) if S == 130 else ((np.arange(S) % 2).astype(np.int32), 2)
    for breaks in (BREAKS7, BREAKS200):
        ref = _reference(hip_ctx, ("cont", S, n), X, cls, "classes", breaks=breaks)
        got = hip_ctx.quantiles(X, PROBS, breaks, cls, n_class)
        _assert_same(got, ref)
        assert got[2][1] + got[2][2] == got[2][0] and np.array_equal(got[4][1] + got[4][2], got[4][0])
    if S == 2:
        assert got[2].tolist() == [1, 0, 1] and np.all(bits(got[0][:, 1]) == NA_REAL_BITS)


@pytest.mark.parametrize("classes", ["one", "five"])
def test_equal_values(hip_ctx, classes):
    """16 rows give tau a few hundred distinct values among 1.1 million pairs, exact zeros among them: every requested
    rank lies inside a run of equal keys, or at its edge."""
    S = 1500
    X = _few_rows(S)
    cls, n_class = (None, 1) if classes == "one" else _five_classes(S)
    ref = _reference(hip_ctx, ("few", S, 16), X, cls, classes, breaks=BREAKS200)
    raw = _matrices(hip_ctx, ("few", S, 16), X)[0][1]
    tri = raw[np.triu_indices(S, k=1)]
    assert len(np.unique(tri[~np.isnan(tri)])) < 1000 and np.any(tri == 0.0)
    _assert_same(hip_ctx.quantiles(X, PROBS, BREAKS200, cls, n_class), ref)


def test_na_pairs(plan_ctx):
    """the constant and the all-missing column (3, 7) are NA with every partner, the single-row column (10) with those
    two: the three as one class, with every other sample a class of its own, leave the within-class group NA pairs alone."""
    X = _edge_matrix()
    S = X.shape[1]
    cls = np.arange(1, S + 1, dtype=np.int32)
    cls[[3, 7, 10]] = 0
    ref = _reference(plan_ctx, "edge", X, cls, "na-class")
    assert ref[2][1] == 0 and ref[3][1] == 3 and ref[3][0] >= 2 * (S - 2) + 1 and ref[7][1:].sum() > 0
    assert np.all(ref[4][1] == 0) and np.all(bits(ref[0][:, 1]) == NA_REAL_BITS)
    for spec in (None, "tkblock=3", "qbatch=1"):
        plan_ctx.debug_set_plan(spec)
        _assert_same(plan_ctx.quantiles(X, PROBS, BREAKS7, cls, S + 1), ref)
    ref1 = _reference(plan_ctx, "edge", X, None, "one")
    _assert_same(plan_ctx.quantiles(X, PROBS, BREAKS7), ref1)


@pytest.mark.parametrize("cfg", [("global", False), ("local", True), ("local", False)])
def test_perspectives_and_scale(hip_ctx, cfg):
    perspective, scale_max = cfg
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _interleaved(S)
    ref = _reference(hip_ctx, ("cont", S, n), X, cls, "classes", perspective=perspective, scale_max=scale_max)
    got = hip_ctx.quantiles(X, PROBS, BREAKS7, cls, n_class, None, perspective, "two.sided", False, 0, scale_max)
    _assert_same(got, ref)
    if not scale_max:
        assert np.array_equal(bits(got[0][0]), bits(got[0][1]))


def test_block_cuts_give_identical_output(plan_ctx):
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _interleaved(S)
    for c, nc, ck in ((None, 1, "one"), (cls, n_class, "classes")):
        ref = _reference(plan_ctx, ("cont", S, n), X, c, ck, breaks=BREAKS200)
        outs = []
        for spec in ("tkblock=1", "tkblock=1000", None):
            plan_ctx.debug_set_plan(spec)
            outs.append(plan_ctx.quantiles(X, PROBS, BREAKS200, c, nc))
            _assert_same(outs[-1], ref)
        for got in outs[1:]:
            _same_bits(got, outs[0])


@pytest.mark.parametrize("case", ["130-classes", "1500-five"])
def test_select_batches_give_identical_output(plan_ctx, case):
    """qbatch=1: one target per batch of eight passes; qbatch=5: several batches of several; the default: one batch"""
    S = int(case.split("-")[0])
    n = 40 if S == 130 else 16
    X = _continuous(S, n) if S == 130 else _few_rows(S)
    cls, n_class = _interleaved(S) if S == 130 else _five_classes(S)
    ref = _reference(plan_ctx, ("cont" if S == 130 else "few", S, n), X, cls, case.split("-")[1], breaks=BREAKS200)
    outs = []
    for spec in ("qbatch=1", "qbatch=5", None):
        plan_ctx.debug_set_plan(spec)
        outs.append(plan_ctx.quantiles(X, PROBS, BREAKS200, cls, n_class))
        _assert_same(outs[-1], ref)
    for got in outs[1:]:
        _same_bits(got, outs[0])
    with pytest.raises(_lib.IciktError, match="qbatch"):
        plan_ctx.debug_set_plan("qbatch=33")


def test_optional_outputs(hip_ctx):
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _interleaved(S)
    full = hip_ctx.quantiles(X, PROBS, BREAKS7, cls, n_class)
    _assert_same(full, _reference(hip_ctx, ("cont", S, n), X, cls, "classes"))
    hist_only = hip_ctx.quantiles(X, (), BREAKS7, cls, n_class)
    assert hist_only[0].shape == (2, 3, 0) and hist_only[1].shape == (3, 0, 2)
    _same_bits(hist_only[2:], full[2:])
    q_only = hip_ctx.quantiles(X, PROBS, None, cls, n_class)
    assert q_only[4].shape == (3, 0) and np.all(q_only[5] == 0)
    _same_bits(q_only[:4], full[:4])
    assert q_only[6] == full[6] and np.array_equal(q_only[7], full[7])
    counts_only = hip_ctx.quantiles(X, (), None, cls, n_class)
    _same_bits(counts_only[2:4], full[2:4])


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.quantiles(X64, *args)
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
    want = _f64_entry(hip_ctx, X64, PROBS, BREAKS7, cls, 3)
    got = hip_ctx.quantiles(X32, PROBS, BREAKS7, cls, 3)
    _same_bits(got, want)
    _assert_same(got, _reference(hip_ctx, "f32", X64, cls, "mod3"))


def test_scipy_csc_matches_dense(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    gna = [np.nan, np.inf, 0.0]
    cls = (np.arange(S) % 3).astype(np.int32)
    want = _f64_entry(hip_ctx, X, PROBS, BREAKS7, cls, 3, gna)
    got = hip_ctx.quantiles(A, PROBS, BREAKS7, cls, 3, gna)
    _same_bits(got, want)
    _assert_same(got, _reference(hip_ctx, "csc", X, cls, "mod3", global_na=gna))


def test_refusals_leave_outputs_and_context_untouched(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.pairs(X)                                   # a prepared matrix and a pair list to keep
    L = _lib.lib()
    E_INVALID = -1
    big = np.zeros((1, 65536), order="F")
    ok_cls = np.zeros(S, dtype=np.int32)
    ok_probs = np.array([0.5, 0.9])
    ok_breaks = np.array([-1.0, 0.0, 1.0])

    def call(Xa, n_feat, n_samp, cls, n_class, probs, breaks, perspective=1, null=None, n_probs=None, n_breaks=None):
        n_probs = len(probs) if n_probs is None else n_probs
        n_breaks = len(breaks) if n_breaks is None else n_breaks
        outs = {"q2": np.full((2, 3, 40), 123.25), "order2": np.full((3, 40, 2), 123.25),
                "n_valid": np.full(3, -7, dtype=np.int64), "n_na": np.full(3, -7, dtype=np.int64),
                "hist": np.full((3, 1100), -7, dtype=np.int64), "outside": np.full((3, 2), -7, dtype=np.int64)}
        mx = np.full(1, 55.5)
        rc5 = np.full(5, -9, dtype=np.int64)
        ptr = {k: (None if k == null else _lib._ptr(v)) for k, v in outs.items()}
        rc = L.icikt_quantiles_f64(hip_ctx._h, _lib._ptr(Xa), n_feat, n_samp, max(n_feat, 1), None, 0, _lib._ptr(cls),
                                   n_class, perspective, 0, 0, 0, 1, _lib._ptr(probs), n_probs, _lib._ptr(breaks),
                                   n_breaks, ptr["q2"], ptr["order2"], ptr["n_valid"], ptr["n_na"], ptr["hist"],
                                   ptr["outside"], _lib._ptr(mx), _lib._ptr(rc5))
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == E_INVALID, rc
        assert msg and b"quantiles" in msg, msg
        assert all(np.all(v == (123.25 if v.dtype == np.float64 else -7)) for v in outs.values())
        assert mx[0] == 55.5 and np.all(rc5 == -9)
        assert hip_ctx.num_pairs() == S * (S - 1) // 2    # the refused call touched nothing
        return msg.decode()

    assert "probs[1] = 1.5" in call(X, n, S, ok_cls, 1, np.array([0.5, 1.5]), ok_breaks)
    assert "probs[0]" in call(X, n, S, ok_cls, 1, np.array([np.nan]), ok_breaks)
    assert "probs[2] = -0." in call(X, n, S, ok_cls, 1, np.array([0.0, 1.0, -0.25]), ok_breaks)
    assert "breaks[2]" in call(X, n, S, ok_cls, 1, ok_probs, np.array([-1.0, 0.0, 0.0, 1.0]))
    assert "breaks[1]" in call(X, n, S, ok_cls, 1, ok_probs, np.array([-1.0, np.inf]))
    assert "ICIKT_QUANTILE_MAX_PROBS" in call(X, n, S, ok_cls, 1, np.full(33, 0.5), ok_breaks)
    assert "ICIKT_HIST_MAX_BINS" in call(X, n, S, ok_cls, 1, ok_probs, np.linspace(-1, 1, 1026))
    assert "ICIKT_HIST_MAX_BINS" in call(X, n, S, ok_cls, 1, ok_probs, np.array([0.0]))
    bad = ok_cls.copy()
    bad[5] = 2
    assert "cls[5] = 2" in call(X, n, S, bad, 2, ok_probs, ok_breaks)
    bad[5] = -1
    assert "cls[5] = -1" in call(X, n, S, bad, 2, ok_probs, ok_breaks)
    assert "ICIKT_TOPK_MAX_SAMPLES" in call(big, 1, 65536, np.zeros(65536, dtype=np.int32), 1, ok_probs, ok_breaks)
    assert "null output (q2)" in call(X, n, S, ok_cls, 1, ok_probs, ok_breaks, null="q2")
    assert "null output (order2)" in call(X, n, S, ok_cls, 1, ok_probs, ok_breaks, null="order2")
    assert "null output (hist)" in call(X, n, S, ok_cls, 1, ok_probs, ok_breaks, null="hist")
    assert "perspective" in call(X, n, S, ok_cls, 1, ok_probs, ok_breaks, perspective=7)
    with pytest.raises(_lib.IciktError, match="quantiles: perspective"):
        hip_ctx.quantiles(X, (0.5,), perspective="sideways")
    with pytest.raises(_lib.IciktError, match=r"quantiles: probs\[0\]"):
        hip_ctx.quantiles(X, (2.0,))
    out, _cnt, rsn = hip_ctx.pairs(X)                  # and the next ordinary call succeeds
    assert out.shape == (S * (S - 1) // 2, 4) and np.all(rsn == 0)


def test_state_after_a_successful_call(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    for cls in (None, (np.arange(S) % 2).astype(np.int32), np.arange(S, dtype=np.int32)):
        hip_ctx.pairs(X)
        got = hip_ctx.quantiles(X, (0.5,), BREAKS7, cls, S)
        assert hip_ctx.num_pairs() == -1
        rc = _lib.lib().icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
        assert rc == -5, rc                            # ICIKT_E_STATE: nothing prepared
    # (the last call: singletons alone -- every pair is a between-class pair)
    assert got[2].tolist() == [28, 0, 28] and np.all(bits(got[0][:, 1]) == NA_REAL_BITS)
    # one column: no pair at all
    one = hip_ctx.quantiles(X[:, :1], (0.5,), BREAKS7)
    assert one[2].tolist() == [0] and one[3].tolist() == [0] and np.all(bits(one[0]) == NA_REAL_BITS)
    assert np.all(one[4] == 0) and one[6] == -np.inf
    out, _cnt, _rsn = hip_ctx.pairs(X)
    assert out.shape[0] == S * (S - 1) // 2


FRONT_BREAKS = np.array([-1.5, -0.3137, -0.0931, 0.0517, 0.2213, 0.3301, 1.5])


def test_front_end_matches_the_checker_engine(hip_ctx):
    """The HIP engine and the CPU oracle agree to 1e-10 on a pair's values, not bitwise (smoke() asserts that bound); a
    quantile is a convex combination of two pair values, so it moves by no more than they do.  Everything that is not
    a float -- groups, counts, the NA pattern, the warnings -- is equal, and so is the histogram, because no reference
    value lies within 1e-10 of a break (asserted on the oracle's values)."""
    from tests.oracle_engine import OracleEngine
    S, n = 130, 40
    X = _continuous(S, n).copy()
    X[:, 17] = 1.5                                     # a constant column: a warning per pair
    cls, _n_class = _interleaved(S)
    labels = [f"batch{k}" for k in cls]
    names = [f"s{i}" for i in range(S)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = api.ici_kendalltau(X, colnames=names, engine=OracleEngine())
    tri = np.asarray(full["raw"])[np.triu_indices(S, k=1)]
    tri = tri[~np.isnan(tri)]
    gap = np.min(np.abs(tri[:, None] - FRONT_BREAKS[None, :]))
    print("closest reference value to a break:", gap)
    assert gap > 1e-10
    res, msgs = [], []
    for eng in (api.HipEngine(), OracleEngine()):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            res.append(api.ici_kendalltau_quantiles(X, probs=PROBS, breaks=FRONT_BREAKS, sample_classes=labels,
                                                    colnames=names, engine=eng))
        msgs.append(sorted(str(x.message) for x in w if str(x.message) in _lib.REASON_WARNINGS.values()))
    got, want = res
    assert msgs[0] == msgs[1] and len(msgs[0]) == S - 1
    assert got["group"] == want["group"] == ["all", "within", "between"]
    assert np.array_equal(got["probs"], want["probs"]) and np.array_equal(got["breaks"], want["breaks"])
    for key in ("n_valid", "n_na", "counts", "n_below", "n_above"):
        assert np.array_equal(got[key], want[key]), key
    assert got["n_na"][0] == S - 1 and got["counts"].shape == (3, 6)
    for key in ("quantile_cor", "quantile_raw"):
        assert got[key].shape == (3, len(PROBS))
        print(key, np.nanmax(np.abs(got[key] - want[key])))
        assert np.array_equal(bits(got[key]) == NA_REAL_BITS, bits(want[key]) == NA_REAL_BITS)
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key]))
        assert np.allclose(got[key], want[key], rtol=0, atol=1e-10, equal_nan=True), key
    assert abs(got["max_taumax"] - want["max_taumax"]) <= 1e-10
