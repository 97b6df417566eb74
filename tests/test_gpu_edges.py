"""icikt_edges_f64 / _in / _csc on the GPU: every pair past a threshold, compacted on the device in combn order.

The reference is the brute-force checker (tests/edges_checker.py) applied to Context.matrix on the same input: i, j,
n_edges and degree must be equal and the five value planes BITWISE equal.  The shapes are the smallest that reach each
part of the compaction: rows shorter than a wave and tiles that hold many rows (S = 65), a row that spans tiles and
several tiles per block (S = 1 500), blocks of one row and blocks that end mid-triangle (tkblock)."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.edges_checker import assert_same, bits, brute_edges

pytestmark = pytest.mark.gpu

_REF = {}   # (data key, perspective, scale_max, alternative, continuity) -> (out5, reason counts): computed once
SENT_I = -7
SENT_D = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]   # a NaN no kernel produces


def _continuous(S, n, seed=11):
    rng = np.random.default_rng(seed + 1000 * S + n)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X


def _matrix(ctx, key, X, global_na=None, perspective="global", scale_max=True, alternative="two.sided",
            continuity=False):
    rk = (key, perspective, scale_max, alternative, continuity)
    if rk not in _REF:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, perspective, alternative, continuity, 0, scale_max, True,
                                      want_keep=False)
        _REF[rk] = (out5, rc5)
    return _REF[rk]


def _triangle(out5, q):
    return out5[q][np.triu_indices(out5.shape[1], k=1)]


def _check_stats(got, out5, rc5):
    """max_taumax and reason_counts against the matrix call's"""
    tm = _triangle(out5, 3)
    tm = tm[~np.isnan(tm)]
    assert got[5] == (tm.max() if tm.size else -np.inf)
    assert np.array_equal(got[6], rc5)


def _raw_call(ctx, X, rule, max_edges, room=None, perspective=1, alternative=0, continuity=0, scale_max=1, null=()):
    """icikt_edges_f64 through ctypes on buffers pre-filled with sentinels (room slots per plane, plane stride
    max_edges as the ABI says: room >= max_edges).  Returns (rc, ei, ej, out5e [5, room], n_edges, degree, mx, rc5)."""
    n, S = X.shape
    room = max(max_edges, 1) if room is None else room
    ei = np.full(room, SENT_I, dtype=np.int32)
    ej = np.full(room, SENT_I, dtype=np.int32)
    out5e = np.full(5 * room, SENT_D, dtype=np.float64)
    n_edges = np.full(1, -99, dtype=np.int64)
    degree = np.full(S, -99, dtype=np.int64)
    mx = np.full(1, 123.0)
    rc5 = np.full(5, -99, dtype=np.int64)
    r = _lib.edge_rule(**rule) if rule is not None else None
    ptr = lambda a, name: None if name in null else _lib._ptr(a)   # noqa: E731
    rc = _lib.lib().icikt_edges_f64(ctx._h, ptr(X, "X"), n, S, n, None, 0, ctypes.byref(r) if r is not None else None,
                                    perspective, alternative, continuity, 0, scale_max, max_edges, ptr(ei, "ei"),
                                    ptr(ej, "ej"), ptr(out5e, "out5e"), ptr(n_edges, "n_edges"), ptr(degree, "degree"),
                                    ptr(mx, "mx"), ptr(rc5, "rc5"))
    return rc, ei, ej, out5e, n_edges, degree, mx, rc5


def _untouched(res):
    _rc, ei, ej, out5e, n_edges, degree, mx, rc5 = res
    return (np.all(ei == SENT_I) and np.all(ej == SENT_I) and np.all(bits(out5e) == bits(SENT_D)) and n_edges[0] == -99
            and np.all(degree == -99) and mx[0] == 123.0 and np.all(rc5 == -99))


@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("S", [2, 3, 65, 130])
def test_small_shapes(hip_ctx, S, n):
    X = _continuous(S, n)
    out5, rc5 = _matrix(hip_ctx, ("cont", S, n), X)
    total = S * (S - 1) // 2
    raw = _triangle(out5, 1)
    thr = float(np.median(raw[~np.isnan(raw)]))
    for rule in ({}, {"min_raw": thr}):
        got = hip_ctx.edges(X, max_edges=total, **rule)
        assert_same(got, brute_edges(out5, **rule))
        _check_stats(got, out5, rc5)
    assert hip_ctx.edges(X, max_edges=total)[3] == total - int(rc5[1:5].sum())


def _thresholds(out5):
    raw = _triangle(out5, 1)
    raw = raw[~np.isnan(raw)]
    return {"all": -1.0, "none": 2.0, "median": float(np.median(raw)), "p99.5": float(np.quantile(raw, 0.995))}


@pytest.mark.parametrize("which", ["all", "none", "median", "p99.5"])
@pytest.mark.parametrize("shape", [(130, 40), (1500, 16)])
def test_thresholds(hip_ctx, shape, which):
    """S = 1 500, n = 16: a row of 1 499 pairs spans tiles, the block holds 1 098 tiles, and 16 rows give tau a few
    hundred distinct values at most, so many raw values equal the threshold itself (>= keeps them)."""
    S, n = shape
    X = _continuous(S, n)
    out5, rc5 = _matrix(hip_ctx, ("cont", S, n), X)
    total = S * (S - 1) // 2
    thr = _thresholds(out5)[which]
    ref = brute_edges(out5, min_raw=thr)
    got = hip_ctx.edges(X, min_raw=thr, max_edges=total)
    assert_same(got, ref)
    _check_stats(got, out5, rc5)
    if which == "all":
        assert got[3] == total - int(rc5[1:5].sum())
    if which == "p99.5":
        assert 0 < got[3] < total // 50
    if which == "none":
        assert got[3] == 0
        res = _raw_call(hip_ctx, X, {"min_raw": thr}, 64)
        assert res[0] == 0 and res[4][0] == 0 and np.all(res[5] == 0)
        assert np.all(res[1] == SENT_I) and np.all(res[2] == SENT_I) and np.all(bits(res[3]) == bits(SENT_D))
    if S == 1500 and which == "median":
        raw = _triangle(out5, 1)
        assert np.sum(raw == thr) > 100                 # (the ties the case is about are there)


def test_block_cuts_give_identical_output(plan_ctx):
    S, n = 130, 40
    X = _continuous(S, n)
    out5, rc5 = _matrix(plan_ctx, ("cont", S, n), X)
    thr = _thresholds(out5)["median"]
    ref = brute_edges(out5, min_raw=thr)
    outs = []
    for spec in ("tkblock=1", "tkblock=1000", None):
        plan_ctx.debug_set_plan(spec)
        outs.append(plan_ctx.edges(X, min_raw=thr, max_edges=S * S))
    for got in outs:
        assert_same(got, ref)
        _check_stats(got, out5, rc5)
        for q in range(3):
            assert got[q].tobytes() == outs[0][q].tobytes()


@pytest.mark.parametrize("spec", [None, "tkblock=1000"])
def test_capacity(plan_ctx, spec):
    S, n = 130, 40
    X = _continuous(S, n)
    out5, _rc5 = _matrix(plan_ctx, ("cont", S, n), X)
    rule = {"min_raw": _thresholds(out5)["median"]}
    ref = brute_edges(out5, **rule)
    n_all = ref[3]
    assert n_all > 1000
    plan_ctx.debug_set_plan(spec)
    for cap in (n_all - 1, 1):
        assert_same(plan_ctx.edges(X, max_edges=cap, **rule), ref, max_edges=cap)
        room = cap + 5
        rc, ei, ej, out5e, n_edges, degree, _mx, _r = _raw_call(plan_ctx, X, rule, cap, room=room)
        assert rc == 0 and n_edges[0] == n_all and np.array_equal(degree, ref[4])
        assert np.array_equal(ei[:cap], ref[0][:cap]) and np.array_equal(ej[:cap], ref[1][:cap])
        assert np.all(ei[cap:] == SENT_I) and np.all(ej[cap:] == SENT_I)
        planes = out5e[:5 * cap].reshape(5, cap)        # the planes lie max_edges apart
        assert np.array_equal(bits(planes), bits(ref[2][:, :cap]))
        assert np.all(bits(out5e[5 * cap:]) == bits(SENT_D))
    # a roomy call that matches fewer than its capacity: the slots behind the edges keep their sentinel
    cap = n_all + 7
    rc, ei, ej, out5e, n_edges, _d, _mx, _r = _raw_call(plan_ctx, X, rule, cap)
    assert rc == 0 and n_edges[0] == n_all
    assert np.array_equal(ei[:n_all], ref[0]) and np.all(ei[n_all:] == SENT_I) and np.all(ej[n_all:] == SENT_I)
    planes = out5e.reshape(5, cap)
    assert np.array_equal(bits(planes[:, :n_all]), bits(ref[2]))
    assert np.all(bits(planes[:, n_all:]) == bits(SENT_D))
    # count only: no output arrays at all
    rc, _ei, _ej, _o, n_edges, degree, _mx, _r = _raw_call(plan_ctx, X, rule, 0, null=("ei", "ej", "out5e"))
    assert rc == 0 and n_edges[0] == n_all and np.array_equal(degree, ref[4])
    got = plan_ctx.edges(X, max_edges=0, **rule)
    assert got[3] == n_all and got[0].shape == (0,) and got[2].shape == (5, 0)


def _edge_matrix():
    rng = np.random.default_rng(5)
    n, S = 40, 12
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    X[:, 3] = 1.25               # constant: reason 3 with every partner
    X[:, 5] = -3.0               # one value again, another one
    X[:, 7] = np.nan             # all missing
    X[:, 10] = np.nan
    X[17, 10] = 0.5              # a single non-missing row: NOT degenerate (its missing rows count as its lowest value)
    return X


@pytest.mark.parametrize("perspective", ["local", "global"])
@pytest.mark.parametrize("spec", [None, "tkblock=1"])
def test_degenerate_columns(plan_ctx, spec, perspective):
    """An all-NaN column (7) and two columns that hold one value in every row (3, 5) are no edge's endpoint.  A column
    with one value and missing cells -- here 10, a single non-missing row -- is an ordinary column under both
    perspectives: its missing rows rank below its value, which makes two groups (the CPU oracle gives reason 0 and a
    number for 9 of its 11 pairs, local and global).  Its edges and its degree are the checker's, not zero."""
    X = _edge_matrix()
    S = X.shape[1]
    out5, rc5 = _matrix(plan_ctx, "edge", X, None, perspective)
    assert rc5[1:5].sum() > 0
    plan_ctx.debug_set_plan(spec)
    for rule in ({}, {"min_raw": -1.0}, {"max_pvalue": 1.0}):
        got = plan_ctx.edges(X, max_edges=S * S, perspective=perspective, **rule)
        assert_same(got, brute_edges(out5, **rule))
        _check_stats(got, out5, rc5)
        assert got[3] == S * (S - 1) // 2 - int(rc5[1:5].sum())
        for col in (3, 5, 7):
            assert got[4][col] == 0 and not np.any(got[0] == col) and not np.any(got[1] == col), col
        assert got[4][10] == S - 1 - 3                 # every partner but the three degenerate columns


@pytest.mark.parametrize("absolute", [False, True])
def test_absolute(hip_ctx, absolute):
    S, n = 65, 40
    X = _continuous(S, n, seed=3) + 1.5 * np.random.default_rng(3).standard_normal((n, 1))   # a shared component ...
    X[:, 1::2] *= -1.0                                 # ... and every odd column negated: raw of both signs
    X = np.asfortranarray(X)
    out5, rc5 = _matrix(hip_ctx, "absolute", X)
    raw = _triangle(out5, 1)
    assert np.sum(raw >= 0.2) > 0 and np.sum(raw <= -0.2) > 0
    rule = {"min_raw": 0.2, "absolute": absolute}
    ref = brute_edges(out5, **rule)
    assert_same(hip_ctx.edges(X, max_edges=S * S, **rule), ref)
    assert ref[3] == int(np.sum((np.abs(raw) if absolute else raw) >= 0.2))


@pytest.mark.parametrize("cfg", [("global", "two.sided", False), ("global", "less", False), ("global", "greater", False),
                                 ("global", "two.sided", True), ("local", "two.sided", False)])
def test_pvalue_and_completeness_bounds(hip_ctx, cfg):
    perspective, alternative, continuity = cfg
    S, n = 65, 40
    X = _continuous(S, n)
    X[:, :20][np.random.default_rng(8).random((n, 20)) < 0.3] = np.nan      # completeness spread over the pairs
    out5, rc5 = _matrix(hip_ctx, "bounds", X, None, perspective, True, alternative, continuity)
    comp = _triangle(out5, 4)
    cthr = float(np.median(comp))
    rules = [{"max_pvalue": 0.05}, {"min_completeness": cthr},
             {"min_raw": 0.0, "max_pvalue": 0.5, "min_completeness": cthr}]
    for rule in rules:
        ref = brute_edges(out5, **rule)
        assert 0 < ref[3] < S * (S - 1) // 2, rule
        got = hip_ctx.edges(X, max_edges=S * S, perspective=perspective, alternative=alternative,
                            continuity=continuity, **rule)
        assert_same(got, ref)
        _check_stats(got, out5, rc5)


def test_two_row_matrix(hip_ctx):
    """n = 2, the case of the ABI's note on a NaN p-value: with and without a p-value bound the edges are the
    checker's on what the matrix call reports, whatever that holds."""
    ctx = hip_ctx
    X = np.asfortranarray(np.array([[1.0, 2.0, 3.0, 1.5], [2.0, 1.0, 4.0, 0.5]]))
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    for rule, n_want in (({}, 6), ({"max_pvalue": 1.0}, 0)):
        got = ctx.edges(X, max_edges=6, **rule)
        assert_same(got, brute_edges(out5, **rule))
        assert got[3] == n_want                        # raw is +-1 and pvalue NaN for all six pairs


def test_scale_max_changes_only_cor(hip_ctx):
    """Tied data (values on a grid of 2/3): every pair's taumax is below 1, so the scale's denominator is not 1 and the
    scaled cor differs from raw (on continuous data max(taumax) is exactly 1 and the two planes are equal)."""
    S, n = 65, 40
    X = np.asfortranarray(np.round(_continuous(S, n) * 1.5) / 1.5)
    thr = _thresholds(_matrix(hip_ctx, "tied", X)[0])["median"]
    res = {}
    for scale_max in (True, False):
        out5, _rc5 = _matrix(hip_ctx, "tied", X, None, "global", scale_max)
        got = hip_ctx.edges(X, min_raw=thr, max_edges=S * S, scale_max=scale_max)
        assert_same(got, brute_edges(out5, min_raw=thr))
        res[scale_max] = got
    assert res[True][5] < 1.0                                       # max_taumax
    a, b = res[True], res[False]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    assert np.array_equal(bits(a[2][1:]), bits(b[2][1:]))
    assert np.array_equal(bits(b[2][0]), bits(b[2][1]))            # unscaled: cor is raw
    assert not np.array_equal(bits(a[2][0]), bits(b[2][0]))


def test_float32_row_major_view_matches_float64(hip_ctx):
    S, n = 65, 40
    rng = np.random.default_rng(21)
    X32 = np.ascontiguousarray(rng.standard_normal((n, S)).astype(np.float32))
    X32[rng.random((n, S)) < 0.08] = np.nan
    assert X32.flags.c_contiguous and _lib.input_view(X32)[2] == _lib.ORDER_ROW
    X64 = np.asfortranarray(X32, dtype=np.float64)
    hip_ctx.f64_entries = True
    try:
        want = hip_ctx.edges(X64, min_raw=0.0, max_edges=S * S)      # icikt_edges_f64
    finally:
        hip_ctx.f64_entries = False
    got = hip_ctx.edges(X32, min_raw=0.0, max_edges=S * S)           # icikt_edges_in
    for q in range(3):
        assert got[q].tobytes() == want[q].tobytes()
    assert got[3] == want[3] and np.array_equal(got[4], want[4]) and got[5] == want[5] and np.array_equal(got[6], want[6])
    assert_same(got, brute_edges(_matrix(hip_ctx, "f32", X64)[0], min_raw=0.0))


def test_csc_view_matches_dense(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    assert _lib.is_sparse(A)
    gna = [np.nan, np.inf, 0.0]
    hip_ctx.f64_entries = True
    try:
        want = hip_ctx.edges(X, min_raw=0.0, max_edges=S * S, global_na=gna)     # icikt_edges_f64, densified
    finally:
        hip_ctx.f64_entries = False
    got = hip_ctx.edges(A, min_raw=0.0, max_edges=S * S, global_na=gna)          # icikt_edges_csc
    for q in range(3):
        assert got[q].tobytes() == want[q].tobytes()
    assert got[3] == want[3] and np.array_equal(got[4], want[4]) and got[5] == want[5] and np.array_equal(got[6], want[6])
    assert_same(got, brute_edges(_matrix(hip_ctx, "csc", X, gna)[0], min_raw=0.0))


def test_argument_errors_touch_nothing(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.pairs(X)                                   # a prepared matrix and a pair list to keep
    rule = {"min_raw": 0.0}
    cases = [("null rule", dict(rule=None, max_edges=4)),
             ("max_edges must not be negative", dict(rule=rule, max_edges=-1, room=4)),
             (r"null output \(ei\)", dict(rule=rule, max_edges=4, null=("ei",))),
             (r"null output \(ej\)", dict(rule=rule, max_edges=4, null=("ej",))),
             (r"null output \(out5e\)", dict(rule=rule, max_edges=4, null=("out5e",))),
             ("edges: perspective", dict(rule=rule, max_edges=4, perspective=7)),
             ("edges: null matrix", dict(rule=rule, max_edges=4, null=("X",)))]
    for msg, kw in cases:
        res = _raw_call(hip_ctx, X, kw.pop("rule"), kw.pop("max_edges"), **kw)
        with pytest.raises(_lib.IciktError, match=msg):
            hip_ctx._chk(res[0], "icikt_edges_f64")
        assert _untouched(res), msg
    with pytest.raises(_lib.IciktError, match="edges: perspective"):
        hip_ctx.edges(X, max_edges=4, perspective="sideways")
    assert hip_ctx.num_pairs() == S * (S - 1) // 2    # refused calls touched nothing
    out, _cnt, rsn = hip_ctx.pairs(X)                  # and the next ordinary call succeeds
    assert out.shape == (S * (S - 1) // 2, 4) and np.all(rsn == 0)


def test_too_many_samples_is_refused(hip_ctx):
    X = np.zeros((1, 65536), order="F")
    res = _raw_call(hip_ctx, X, {"min_raw": 0.0}, 4)
    with pytest.raises(_lib.IciktError, match="ICIKT_TOPK_MAX_SAMPLES"):
        hip_ctx._chk(res[0], "icikt_edges_f64")
    assert _untouched(res)


def test_state_after_a_successful_call(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.edges(X, min_raw=0.0, max_edges=5)
    assert hip_ctx.num_pairs() == -1
    rc = _lib.lib().icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
    assert rc == -5, rc                                # ICIKT_E_STATE: nothing prepared
    out, _cnt, _rsn = hip_ctx.pairs(X)
    assert out.shape[0] == S * (S - 1) // 2


def test_timing_flag_accounts_the_compaction_under_the_epilogue(hip_ctx):
    S, n = 65, 40
    X = _continuous(S, n)
    hip_ctx.reset_timers()
    hip_ctx.edges(X, min_raw=0.0, max_edges=S * S, flags=_lib.FLAG_TIMING)
    ms, spans = hip_ctx.kernel_ms(_lib.K_EPILOGUE)
    assert spans >= 2 and ms > 0.0
    hip_ctx.reset_timers()


def _front_end_data():
    S, n = 12, 300
    rng = np.random.default_rng(33)
    X = rng.standard_normal((n, S))
    X[rng.random((n, S)) < 0.08] = np.nan
    X[X > 2.2] = 0.0                                   # zeros: missing under the default global_na
    return X, [f"s{i}" for i in range(S)]


def test_front_end_matches_the_oracle_engine(hip_ctx):
    from tests.oracle_engine import OracleEngine
    X, names = _front_end_data()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = api.ici_kendalltau(X, colnames=names, engine=OracleEngine())
    raw = np.sort(np.asarray(full["raw"])[np.triu_indices(len(names), k=1)])
    # the engines agree to 1e-10, not bitwise: the threshold sits in the middle of a gap wider than 1e-6 between
    # neighbouring sorted oracle values, the first such gap from the 90th percentile on
    at = next(q for q in range(int(0.9 * raw.size), raw.size - 1) if raw[q + 1] - raw[q] > 1e-6)
    thr = 0.5 * (raw[at] + raw[at + 1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = api.ici_kendalltau_edges(X, min_raw=thr, colnames=names, engine=api.HipEngine())
        want = api.ici_kendalltau_edges(X, min_raw=thr, colnames=names, engine=OracleEngine())
    assert want["n_edges"] == raw.size - 1 - at and want["n_edges"] > 0
    assert got["n_edges"] == want["n_edges"]
    for key in ("i", "j", "s1", "s2", "degree"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("cor", "raw", "pvalue", "taumax", "completeness"):
        assert np.allclose(got[key], want[key], rtol=0, atol=1e-10), (key, np.max(np.abs(got[key] - want[key])))
    assert abs(got["max_taumax"] - want["max_taumax"]) <= 1e-10


def test_automatic_second_call(hip_ctx, monkeypatch):
    X, names = _front_end_data()
    eng = api.HipEngine()
    calls = []
    inner = eng.edges

    def counting(*a, **kw):
        calls.append(a[5])                             # max_edges
        return inner(*a, **kw)

    eng.edges = counting
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        roomy = api.ici_kendalltau_edges(X, min_raw=0.0, colnames=names, engine=eng)
        assert len(calls) == 1 and roomy["n_edges"] > 3
        monkeypatch.setattr(api, "EDGES_DEFAULT_CAPACITY", 3)
        monkeypatch.setattr(api, "EDGES_CAPACITY_PER_SAMPLE", 0)
        del calls[:]
        tight = api.ici_kendalltau_edges(X, min_raw=0.0, colnames=names, engine=eng)
        assert calls == [3, roomy["n_edges"]]
        cut = api.ici_kendalltau_edges(X, min_raw=0.0, max_edges=3, colnames=names, engine=eng)
    for key in ("i", "j", "s1", "s2", "degree", "cor", "raw", "pvalue", "taumax", "completeness"):
        assert np.array_equal(tight[key], roomy[key]), key
        if key != "degree":
            assert np.array_equal(cut[key], roomy[key][:3]), key
    assert tight["n_edges"] == roomy["n_edges"] == cut["n_edges"]
    assert np.array_equal(cut["degree"], roomy["degree"])
