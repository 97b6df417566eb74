"""icikt_cross_f64 / _in on the GPU: the query x reference rectangle, as five matrices and as every query's k best
reference columns.

The yardstick is Context.matrix on the stacked matrix [query, reference] with the rectangle's explicit pair list
(i = q, j = Sq + r), on a context created for it, then the brute-force checker (tests/cross_checker.py): integers must
be equal and doubles BITWISE equal, the NA_real_ padding included.  cor is comparable bit for bit too: with that pair
list the matrix entry scales by the largest taumax of the rectangle.  The shapes are the smallest that reach each part:
an odd and an even number of query columns (with and without the padding column), one and several 256-wide passes over
a query's row, more than one sort round, full 256-entry lists, blocks of one row and blocks of several."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests import stream_cases as sc
from tests.cross_checker import KEYS, assert_topk_same, bits, brute_cross_topk, max_taumax, rect_block, rect_pairs
from tests.topk_checker import NA_REAL_BITS

pytestmark = pytest.mark.gpu

E_INVALID = -1
_YARD = {}   # (data key, global_na, perspective, scale_max, alternative, continuity) -> (rect5, reason counts): computed once


def _continuous(Sq, Sr, n, seed=17):
    rng = np.random.default_rng(seed + 1000 * Sq + 10 * Sr + n)
    X = np.asfortranarray(rng.standard_normal((n, Sq + Sr)))
    X[rng.random((n, Sq + Sr)) < 0.08] = np.nan
    return np.asfortranarray(X[:, :Sq]), np.asfortranarray(X[:, Sq:])


def _yardstick(key, Q, R, global_na=None, perspective="global", scale_max=True, alternative="two.sided",
               continuity=False):
    yk = (key, None if global_na is None else tuple(map(str, global_na)), perspective, scale_max, alternative, continuity)
    if yk not in _YARD:
        Sq, Sr = Q.shape[1], R.shape[1]
        X = np.asfortranarray(np.hstack([np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64)]))
        pi, pj = rect_pairs(Sq, Sr)
        ctx = _lib.Context(0)
        try:
            out5, _keep, rc5 = ctx.matrix(X, global_na, pi, pj, perspective, alternative, continuity, 0, scale_max, True,
                                          want_keep=False)
        finally:
            ctx.close()
        _YARD[yk] = (rect_block(out5, Sq), rc5)
    return _YARD[yk]


def _assert_cross(got, rect5, rc5, k):
    """Everything a call returned against the yardstick's rectangle (got: Context.cross' tuple)."""
    out5, idx, vals, n_valid, mx, rc = got
    if out5 is not None:
        assert out5.shape == rect5.shape
        for f, key in enumerate(KEYS):
            assert np.array_equal(bits(out5[f]), bits(rect5[f])), key
    if k is not None:
        assert_topk_same(idx, vals, n_valid, brute_cross_topk(rect5, k))
    assert mx == max_taumax(rect5)
    assert np.array_equal(rc, rc5)


def _same_results(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray) and x.dtype == np.float64:
            assert np.array_equal(bits(x), bits(y))
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        else:
            assert x == y or (x is None and y is None)


@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (3, 5), (4, 64), (5, 65), (7, 130)])
def test_small_shapes(hip_ctx, shape, n):
    Sq, Sr = shape
    Q, R = _continuous(Sq, Sr, n)
    rect5, rc5 = _yardstick(("cont", Sq, Sr, n), Q, R)
    k = min(7, Sr + 1)
    got = hip_ctx.cross(Q, R, k)                      # planes and top-k in one call
    _assert_cross(got, rect5, rc5, k)
    assert got[1].shape == (Sq, k) and got[3].shape == (Sq,)


@pytest.mark.parametrize("k", ["1", "7", "Sr-1", "Sr", "Sr+5"])
def test_k_edges(hip_ctx, k):
    Sq, Sr, n = 5, 65, 40
    Q, R = _continuous(Sq, Sr, n)
    k = {"1": 1, "7": 7, "Sr-1": Sr - 1, "Sr": Sr, "Sr+5": Sr + 5}[k]
    rect5, rc5 = _yardstick(("cont", Sq, Sr, n), Q, R)
    got = hip_ctx.cross(Q, R, k, want_matrix=False)
    _assert_cross(got, rect5, rc5, k)
    assert np.array_equal(got[3], np.full(Sq, min(k, Sr)))


def test_cap_full_lists(hip_ctx):
    Sq, Sr, n, k = 3, 300, 50, 256
    Q, R = _continuous(Sq, Sr, n)
    rect5, rc5 = _yardstick(("cont", Sq, Sr, n), Q, R)
    got = hip_ctx.cross(Q, R, k, want_matrix=False)
    _assert_cross(got, rect5, rc5, k)
    assert np.all(got[3] == 256)


@pytest.mark.parametrize("k", [5, 100])
def test_many_candidates_and_index_ties(hip_ctx, k):
    """1 500 candidates per query: several 256-wide passes and more than one sort round; 16 rows give tau a few hundred
    distinct values at most, so every query has reference columns of equal raw and the index decides."""
    Sq, Sr, n = 3, 1500, 16
    Q, R = _continuous(Sq, Sr, n)
    rect5, rc5 = _yardstick(("cont", Sq, Sr, n), Q, R)
    raw_row = rect5[1][0]
    assert len(np.unique(raw_row[~np.isnan(raw_row)])) < 1000      # (the ties the case is about are there)
    _assert_cross(hip_ctx.cross(Q, R, k, want_matrix=False), rect5, rc5, k)


def test_block_cuts_give_identical_output(plan_ctx):
    """tkblock=1: a query row per block, every row unpaired; 66: blocks of two rows and a trailing single row; 100:
    the same cut by a budget that is no multiple of the row; default: one block."""
    Sq, Sr, n, k = 5, 33, 40, 7
    Q, R = _continuous(Sq, Sr, n)
    rect5, rc5 = _yardstick(("cont", Sq, Sr, n), Q, R)
    outs = []
    for spec in ("tkblock=1", "tkblock=66", "tkblock=100", None):
        plan_ctx.debug_set_plan(spec)
        outs.append(plan_ctx.cross(Q, R, k))
    for got in outs:
        _assert_cross(got, rect5, rc5, k)
        _same_results(got, outs[0])


def _na_matrices():
    rng = np.random.default_rng(6)
    n = 40
    Q = np.asfortranarray(rng.standard_normal((n, 4)))
    R = np.asfortranarray(rng.standard_normal((n, 9)))
    Q[rng.random(Q.shape) < 0.08] = np.nan
    R[rng.random(R.shape) < 0.08] = np.nan
    Q[:, 1] = 1.25               # constant: reason 3 with every reference column
    Q[:, 3] = np.nan             # all missing
    R[:, 2] = -0.5               # the same on the reference side
    R[:, 6] = np.nan
    R[:, 8] = R[:, 4]            # equal raw for every query: the index decides
    return Q, R


@pytest.mark.parametrize("spec", [None, "tkblock=1"])
def test_na_pairs(plan_ctx, spec):
    Q, R = _na_matrices()
    Sr = R.shape[1]
    rect5, rc5 = _yardstick("na", Q, R)
    plan_ctx.debug_set_plan(spec)
    got = plan_ctx.cross(Q, R, Sr)
    _assert_cross(got, rect5, rc5, Sr)
    _out5, idx, vals, n_valid, _mx, rc = got
    assert n_valid.tolist() == [Sr - 2, 0, Sr - 2, 0]
    assert np.all(idx[[1, 3]] == -1) and np.all(bits(vals[:, [1, 3]]) == NA_REAL_BITS)
    assert not np.any(np.isin(idx, (2, 6)))           # a constant or all-missing reference column is never a partner
    assert rc.sum() == Q.shape[1] * Sr and rc[0] == 2 * (Sr - 2)
    for q in (0, 2):
        row = idx[q].tolist()
        assert row.index(4) < row.index(8) and bits(vals[1, q])[row.index(4)] == bits(vals[1, q])[row.index(8)]


@pytest.mark.parametrize("cfg", [("global", True, "two.sided", False), ("local", True, "two.sided", False),
                                 ("global", False, "two.sided", False), ("local", False, "less", True),
                                 ("global", True, "greater", True)])
def test_arguments(hip_ctx, cfg):
    """Both perspectives, scale_max on and off, a non-default alternative with continuity, and a global_na list with
    NaN, Inf, 0 and 5 that both matrices hold."""
    perspective, scale_max, alternative, continuity = cfg
    rng = np.random.default_rng(8)
    n = 60
    Q = np.asfortranarray(rng.integers(0, 12, size=(n, 3)).astype(np.float64))
    R = np.asfortranarray(rng.integers(0, 12, size=(n, 6)).astype(np.float64))
    for M in (Q, R):
        M[rng.random(M.shape) < 0.05] = np.nan
        M[rng.random(M.shape) < 0.05] = np.inf
    assert all(np.any(M == v) for M in (Q, R) for v in (0.0, 5.0, np.inf)) and np.isnan(Q).any() and np.isnan(R).any()
    gna = (float("nan"), float("inf"), 0.0, 5.0)
    rect5, rc5 = _yardstick("args", Q, R, gna, perspective, scale_max, alternative, continuity)
    got = hip_ctx.cross(Q, R, 4, True, gna, perspective, alternative, continuity, 0, scale_max)
    _assert_cross(got, rect5, rc5, 4)
    plain, _rc = _yardstick("args", Q, R, None, perspective, scale_max, alternative, continuity)
    assert not np.array_equal(bits(plain[1]), bits(rect5[1]))     # (the list changes the answer: it was applied)


def test_views_of_different_type_and_order(hip_ctx):
    """A row-major float32 query with a column-major float64 reference whose ld exceeds n, and a row-major int32
    reference with a column-major float64 query: each equals the result on float64 copies."""
    rng = np.random.default_rng(23)
    n, Sq, Sr, k = 40, 5, 12, 6
    Q32 = np.ascontiguousarray(rng.standard_normal((n, Sq)).astype(np.float32))
    Q32[rng.random((n, Sq)) < 0.08] = np.nan
    big = np.asfortranarray(rng.standard_normal((n + 7, Sr)))
    big[rng.random(big.shape) < 0.08] = np.nan
    Rv = big[:n, :]
    assert _lib.input_view(Q32)[1:4] == (_lib.DTYPE_F32, _lib.ORDER_ROW, Sq)
    assert _lib.input_view(Rv)[1:5] == (_lib.DTYPE_F64, _lib.ORDER_COL, n + 7, False)
    Q64, R64 = np.asfortranarray(Q32, dtype=np.float64), np.asfortranarray(Rv)
    want = hip_ctx.cross(Q64, R64, k)
    _same_results(hip_ctx.cross(Q32, Rv, k), want)
    _assert_cross(want, *_yardstick("views-f32", Q64, R64), k)

    Ri = np.ascontiguousarray(rng.integers(-20, 20, size=(n, Sr)).astype(np.int32))
    Qv = big[3:n + 3, :Sq]
    assert _lib.input_view(Ri)[1:4] == (_lib.DTYPE_I32, _lib.ORDER_ROW, Sr)
    assert _lib.input_view(Qv)[1:5] == (_lib.DTYPE_F64, _lib.ORDER_COL, n + 7, False)
    Qc, Rc = np.asfortranarray(Qv), np.asfortranarray(Ri, dtype=np.float64)
    want = hip_ctx.cross(Qc, Rc, k)
    _same_results(hip_ctx.cross(Qv, Ri, k), want)
    _assert_cross(want, *_yardstick("views-i32", Qc, Rc), k)


def test_f64_entry_matches_the_view_entry(hip_ctx):
    Q, R = _continuous(5, 65, 40)
    want = hip_ctx.cross(Q, R, 7)
    hip_ctx.f64_entries = True
    try:
        got = hip_ctx.cross(Q, R, 7)
    finally:
        hip_ctx.f64_entries = False
    _same_results(got, want)


def test_output_subsets(hip_ctx):
    Sq, Sr, n, k = 5, 65, 40, 7
    Q, R = _continuous(Sq, Sr, n)
    rect5, rc5 = _yardstick(("cont", Sq, Sr, n), Q, R)
    planes = hip_ctx.cross(Q, R)                           # planes only
    assert planes[1] is None and planes[2] is None and planes[3] is None
    _assert_cross(planes, rect5, rc5, None)
    lists = hip_ctx.cross(Q, R, k, want_matrix=False)      # top-k only
    assert lists[0] is None
    _assert_cross(lists, rect5, rc5, k)
    # n_valid alone, through the C entry: every top-k output is optional on its own
    nv = np.full(Sq, -9, dtype=np.int32)
    rc = _lib.lib().icikt_cross_f64(hip_ctx._h, _lib._ptr(Q), n, _lib._ptr(R), n, n, Sq, Sr, None, 0, k, 1, 0, 0, 0, 1, None,
                                    None, None, _lib._ptr(nv), None, None)
    assert rc == 0 and np.array_equal(nv, lists[3])


def test_empty_sides(hip_ctx):
    Q, R = _continuous(3, 5, 40)
    out5, idx, vals, n_valid, mx, rc = hip_ctx.cross(Q[:, :0], R, 2)
    assert out5.shape == (5, 0, 5) and idx.shape == (0, 2) and n_valid.shape == (0,) and mx == -np.inf and rc.sum() == 0
    out5, idx, vals, n_valid, mx, rc = hip_ctx.cross(Q, R[:, :0], 2)
    assert out5.shape == (5, 3, 0) and mx == -np.inf and rc.sum() == 0
    assert np.all(idx == -1) and np.all(bits(vals) == NA_REAL_BITS) and n_valid.tolist() == [0, 0, 0]
    _assert_cross(hip_ctx.cross(Q, R, 2), *_yardstick(("cont", 3, 5, 40), Q, R), 2)


def _raw_call(ctx, Q, R, n, Sq, Sr, k, out5=None, idx=None, vals=None, n_valid=None, mx=None, rc5=None):
    return _lib.lib().icikt_cross_f64(ctx._h, _lib._ptr(Q), n, _lib._ptr(R), n, n, Sq, Sr, None, 0, k, 1, 0, 0, 0, 1,
                                      _lib._ptr(out5), _lib._ptr(idx), _lib._ptr(vals), _lib._ptr(n_valid), _lib._ptr(mx),
                                      _lib._ptr(rc5))


def _message(ctx):
    return (_lib.lib().icikt_last_error(ctx._h) or b"").decode()


def test_refusals_touch_nothing(hip_ctx):
    n, Sq, Sr, k = 30, 3, 8, 4
    Q, R = _continuous(Sq, Sr, n)
    X = np.asfortranarray(np.hstack([Q, R]))
    hip_ctx.pairs(X)                                   # a prepared matrix and a pair list to keep
    kept = hip_ctx.num_pairs()
    idx = np.full((Sq, k), -7, dtype=np.int32)
    vals = np.full((5, Sq, k), -7.0)
    mx = np.full(1, -7.0)
    rc5 = np.full(5, -7, dtype=np.int64)
    # more columns than the limit, with the small buffers above: the check precedes every allocation and every read
    for big_q, big_r in ((3, 65533), (4, 65532), (65535, 1), (40000, 40000)):
        assert big_q + (big_q & 1) + big_r > _lib.TOPK_MAX_SAMPLES
        assert _raw_call(hip_ctx, Q, R, n, big_q, big_r, k, idx=idx, vals=vals, mx=mx, rc5=rc5) == E_INVALID
        assert "ICIKT_TOPK_MAX_SAMPLES" in _message(hip_ctx) and "65535" in _message(hip_ctx)
    for bad_k in (0, 257):
        assert _raw_call(hip_ctx, Q, R, n, Sq, Sr, bad_k, idx=idx, vals=vals, mx=mx, rc5=rc5) == E_INVALID
        assert "cross: k must be in 1 .. ICIKT_TOPK_MAX" in _message(hip_ctx)
    assert _raw_call(hip_ctx, Q, R, n, Sq, Sr, k) == E_INVALID
    assert "cross: all outputs are null" in _message(hip_ctx)
    assert _raw_call(hip_ctx, None, R, n, Sq, Sr, k, idx=idx) == E_INVALID
    assert "cross (query): null matrix" in _message(hip_ctx)
    assert _raw_call(hip_ctx, Q, None, n, Sq, Sr, k, idx=idx) == E_INVALID
    assert "cross (reference): null matrix" in _message(hip_ctx)
    with pytest.raises(_lib.IciktError, match="cross: perspective"):
        hip_ctx.cross(Q, R, k, perspective="sideways")
    with pytest.raises(ValueError, match="share their features"):
        hip_ctx.cross(Q[:20], R, k)
    with pytest.raises(_lib.IciktError, match="ICIKT_TOPK_MAX_SAMPLES"):
        hip_ctx.cross(np.zeros((1, 3), order="F"), np.zeros((1, 65533), order="F"), 1)
    assert np.all(idx == -7) and np.all(vals == -7.0) and mx[0] == -7.0 and np.all(rc5 == -7)
    assert hip_ctx.num_pairs() == kept                 # refused calls touched nothing
    # and the same context then serves a correct call
    _assert_cross(hip_ctx.cross(Q, R, k), *_yardstick(("cont", Sq, Sr, n), Q, R), k)
    assert hip_ctx.num_pairs() == -1                   # which leaves neither a prepared matrix nor a pair list behind
    assert _lib.lib().icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, None, None, None) == -5


def test_stale_context():
    """cross after a larger topk call, after hclust and after a smaller cross, then matrix after cross: each result
    equals that of a fresh context."""
    Sq, Sr, n, k = 5, 65, 40, 7
    Q, R = _continuous(Sq, Sr, n)
    rect5, rc5 = _yardstick(("cont", Sq, Sr, n), Q, R)
    Qs, Rs = _continuous(3, 5, 40)
    small = _yardstick(("cont", 3, 5, 40), Qs, Rs)
    big = np.asfortranarray(np.random.default_rng(3).standard_normal((60, 200)))
    X = np.asfortranarray(np.hstack([Q, R]))
    fresh = _lib.Context(0)
    try:
        want_matrix = fresh.matrix(X, None, None, None, want_keep=False)
    finally:
        fresh.close()
    ctx = _lib.Context(0)
    try:
        ctx.topk(big, 9)
        _assert_cross(ctx.cross(Q, R, k), rect5, rc5, k)
        ctx.hclust(big[:, :130], "average")
        _assert_cross(ctx.cross(Q, R, k), rect5, rc5, k)
        _assert_cross(ctx.cross(Qs, Rs, 2), *small, 2)
        _assert_cross(ctx.cross(Q, R, k), rect5, rc5, k)
        got = ctx.matrix(X, None, None, None, want_keep=False)
        assert np.array_equal(bits(got[0]), bits(want_matrix[0])) and np.array_equal(got[2], want_matrix[2])
    finally:
        ctx.close()


def test_on_a_caller_stream():
    """One call on a caller's side stream that is still busy: the entry may not return before the stream has reached
    it, and its result is the yardstick's."""
    import torch
    from tests.test_gpu_caller_stream import HOST_GATE_S, Gate, Lane
    X = sc.true_matrix(sc.Case(700, "continuous"))
    Q, R = np.asfortranarray(X[:, :3]), np.asfortranarray(X[:, 3:])
    rect5, rc5 = _yardstick("stream", Q, R)
    gate = Gate()
    ctx = _lib.Context(0)
    try:
        lane = Lane(ctx, "side")
        lane.warm(gate)
        with torch.cuda.stream(lane.ts):
            gate.run(gate.seconds(HOST_GATE_S))
            e_gate = torch.cuda.Event()
            e_gate.record()
            held = not e_gate.query()
        got = ctx.cross(Q, R, 4)
        assert held, "the gate was over before the call"
        assert e_gate.query(), "returned before the stream it was told to use had reached it"
        _assert_cross(got, rect5, rc5, 4)
    finally:
        ctx.close()


def test_front_end_matches_the_oracle_engine(hip_ctx):
    from tests.oracle_engine import OracleEngine
    rng = np.random.default_rng(34)
    n, Sq, Sr, k = 300, 4, 9, 5
    X = rng.standard_normal((n, Sq + Sr))
    X[rng.random(X.shape) < 0.08] = np.nan
    X[X > 2.2] = 0.0                                   # zeros: missing under the default global_na
    Q, R = X[:, :Sq], X[:, Sq:]
    qn, rn = [f"q{i}" for i in range(Sq)], [f"r{j}" for j in range(Sr)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = api.ici_kendalltau_cross(Q, R, k=k, query_names=qn, reference_names=rn, engine=api.HipEngine())
        want = api.ici_kendalltau_cross(Q, R, k=k, query_names=qn, reference_names=rn, engine=OracleEngine())
    assert np.array_equal(got["indices"], want["indices"])
    assert np.array_equal(got["n_valid"], want["n_valid"])
    assert np.array_equal(got["neighbors"], want["neighbors"])
    for key in KEYS:
        for name in (key, "topk_" + key):
            a, b = np.asarray(got[name]), np.asarray(want[name])
            assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
            assert np.allclose(a, b, rtol=0, atol=1e-10, equal_nan=True), name      # (the oracle's tolerance, as for topk)
    assert abs(got["max_taumax"] - want["max_taumax"]) <= 1e-10
