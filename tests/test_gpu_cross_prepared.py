"""icikt_ref_prepare_* / icikt_ref_cross_* on the GPU: a reference that stays prepared on its context, batch after batch
of query columns against it, and every query's median to every class of a labelled reference.

The yardstick is never the code under test.  For the rectangle it is Context.cross -- both matrices uploaded with the
call, the query first -- on a context of its own: integers must be equal and doubles BITWISE equal, the NA_real_ padding
included, in all six returned items.  For the class tables it is the plain-loop checker (tests/cross_class_checker.py)
applied to the five matrices of that call.  The shapes are the smallest that reach each part: Sr odd and even (with and
without the padding column behind the reference), Sq odd and even, batches narrower than an earlier one, blocks of one
query row and of several, columns long enough for the tie verdict to be read back, cells past the 4 096-key LDS stage."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests import stream_cases as sc
from tests.classmat_checker import clear_nearest, interleaved, signal_matrix
from tests.cross_checker import KEYS, bits
from tests.cross_class_checker import NA_REAL_BITS, brute_cross_class, nearest

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
CAP = 8


@pytest.fixture(scope="module")
def yard():
    """the yardstick's context: Context.cross, nothing else"""
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture
def ref_ctx():
    ctx = _lib.Context(0)
    yield ctx
    ctx.debug_set_plan(None)
    ctx.close()


def _continuous(Sq, Sr, n, seed=29):
    rng = np.random.default_rng(seed + 1000 * Sq + 10 * Sr + n)
    X = np.asfortranarray(rng.standard_normal((n, Sq + Sr)))
    X[rng.random((n, Sq + Sr)) < 0.08] = np.nan
    return np.asfortranarray(X[:, :Sq]), np.asfortranarray(X[:, Sq:])


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray) and x.dtype == np.float64:
            assert x.shape == y.shape and np.array_equal(bits(x), bits(y))
        elif isinstance(x, np.ndarray):
            assert x.shape == y.shape and np.array_equal(x, y)
        else:
            assert x == y or (x is None and y is None)


def _assert_classes(got, rect5, cls, n_class):
    """med2 and n_valid of a cross_prepared tuple against the checker on the yardstick's matrices"""
    want2, want_n = brute_cross_class(rect5, cls, n_class)
    assert got[6].shape == want2.shape and got[7].shape == want_n.shape
    assert np.array_equal(got[7], want_n)
    assert np.array_equal(bits(got[6]), bits(want2))
    return want2, want_n


def _check(ctx, yard, Q, R, k, cls=None, n_class=0, global_na=None, perspective="global", alternative="two.sided",
           continuity=False, scale_max=True):
    """One batch on the context's prepared reference against Context.cross of the yardstick's context"""
    got = ctx.cross_prepared(Q, k, True, cls, n_class, perspective, alternative, continuity, 0, scale_max)
    want = yard.cross(Q, R, k, True, global_na, perspective, alternative, continuity, 0, scale_max)
    _same_results(got[:6], want)
    if cls is not None:
        _assert_classes(got, want[0], cls, n_class)
    else:
        assert got[6] is None and got[7] is None
    return got, want


# ---- shapes, batches, state ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("shape", [(1, 1), (2, 1), (1, 2), (3, 5), (4, 64), (5, 65), (7, 130)])
def test_small_shapes(hip_ctx, yard, shape, n):
    Sq, Sr = shape
    Q, R = _continuous(Sq, Sr, n)
    hip_ctx.prepare_reference(R, CAP)
    assert hip_ctx.reference_info() == (n, Sr, CAP)
    got, _want = _check(hip_ctx, yard, Q, R, min(7, Sr + 1))
    assert got[0].shape == (5, Sq, Sr) and got[1].shape == (Sq, min(7, Sr + 1))


@pytest.mark.parametrize("Sr", [65, 130])
def test_batches_in_sequence_on_one_reference(ref_ctx, yard, Sr):
    """7 columns, then 2, then 5, then the capacity: no column left over from a wider batch, no pair list or verdict
    kept too long -- each batch is its own fresh Context.cross."""
    pool, R = _continuous(22, Sr, 40)
    cls = (np.arange(Sr) % 3).astype(np.int32)
    ref_ctx.prepare_reference(R, CAP)
    at = 0
    for Sq in (7, 2, 5, CAP):
        _check(ref_ctx, yard, np.asfortranarray(pool[:, at:at + Sq]), R, 4, cls, 3)
        at += Sq
    assert ref_ctx.reference_info() == (40, Sr, CAP)
    assert ref_ctx.num_pairs() == -1                   # the device-resident calls see nothing of it
    assert _lib.lib().icikt_run_dev(ref_ctx._h, 1, 0, 0, 0, None, None, None) == E_STATE


def _raw_call(ctx, Q, n, Sq, k, cls=None, n_class=0, persp=1, out5=None, idx=None, vals=None, n_valid=None, med2=None,
              cls_n=None, mx=None, rc5=None):
    p = _lib._ptr
    return _lib.lib().icikt_ref_cross_f64(ctx._h, p(Q), n, n, Sq, k, p(cls), n_class, persp, 0, 0, 0, 1, p(out5), p(idx),
                                          p(vals), p(n_valid), p(med2), p(cls_n), p(mx), p(rc5))


def _message(ctx):
    return (_lib.lib().icikt_last_error(ctx._h) or b"").decode()


class _Sentinels:
    def __init__(self, Sq, Sr, k, C):
        self.out5 = np.full((5, Sq, Sr), -7.0)
        self.idx = np.full((Sq, k), -7, dtype=np.int32)
        self.vals = np.full((5, Sq, k), -7.0)
        self.n_valid = np.full(Sq, -7, dtype=np.int32)
        self.med2 = np.full((2, C, Sq), -7.0)
        self.cls_n = np.full((C, Sq), -7, dtype=np.int32)
        self.mx = np.full(1, -7.0)
        self.rc5 = np.full(5, -7, dtype=np.int64)

    def kw(self):
        return dict(out5=self.out5, idx=self.idx, vals=self.vals, n_valid=self.n_valid, med2=self.med2, cls_n=self.cls_n,
                    mx=self.mx, rc5=self.rc5)

    def untouched(self):
        return all(np.all(a == -7) for a in self.kw().values())


def test_capacity_and_state(ref_ctx, yard):
    n, Sr, k, C = 40, 33, 4, 3
    pool, R = _continuous(12, Sr, n)
    Q = np.asfortranarray(pool[:, :5])
    wide = np.asfortranarray(pool[:, :CAP + 1])
    cls = (np.arange(Sr) % C).astype(np.int32)
    s = _Sentinels(CAP + 1, Sr, k, C)
    # no reference yet
    assert _raw_call(ref_ctx, Q, n, 5, k, **s.kw()) == E_STATE and "no prepared reference" in _message(ref_ctx)
    assert _lib.lib().icikt_ref_info(ref_ctx._h, None, None, None) == E_STATE
    with pytest.raises(_lib.IciktError):
        ref_ctx.cross_prepared(Q, k)
    # refused preparations: nothing is prepared by them
    p = _lib._ptr
    for cap in (0, -3):
        assert _lib.lib().icikt_ref_prepare_f64(ref_ctx._h, p(R), n, n, Sr, cap, None, 0, 0) == E_INVALID
        assert "query_capacity must be at least 1" in _message(ref_ctx)
    for big_r, cap in ((65535, 1), (65533, 2), (65532, 3), (3, 65533), (40000, 40000)):
        assert _lib.lib().icikt_ref_prepare_f64(ref_ctx._h, p(R), n, n, big_r, cap, None, 0, 0) == E_INVALID
        assert "ICIKT_TOPK_MAX_SAMPLES" in _message(ref_ctx) and "65535" in _message(ref_ctx)
    assert _lib.lib().icikt_ref_prepare_f64(ref_ctx._h, None, n, n, Sr, CAP, None, 0, 0) == E_INVALID
    assert _raw_call(ref_ctx, Q, n, 5, k, **s.kw()) == E_STATE

    ref_ctx.prepare_reference(R, CAP)
    _check(ref_ctx, yard, Q, R, k, cls, C)
    # a batch over the capacity, other rows, and the refusals of icikt_cross_*: nothing is written, the reference stays
    assert _raw_call(ref_ctx, wide, n, CAP + 1, k, cls, C, **s.kw()) == E_INVALID
    assert "exceeds the query_capacity" in _message(ref_ctx) and "(8)" in _message(ref_ctx)
    assert _raw_call(ref_ctx, Q, n - 1, 5, k, cls, C, **s.kw()) == E_INVALID
    assert "the prepared reference has 40 rows" in _message(ref_ctx)
    for bad_k in (0, 257):
        assert _raw_call(ref_ctx, Q, n, 5, bad_k, cls, C, **s.kw()) == E_INVALID
        assert "ref_cross: k must be in 1 .. ICIKT_TOPK_MAX" in _message(ref_ctx)
    for bad_c in (0, 65536):
        assert _raw_call(ref_ctx, Q, n, 5, k, cls, bad_c, **s.kw()) == E_INVALID
        assert "n_class must be in 1 .. 65535" in _message(ref_ctx)
    bad = cls.copy()
    bad[20] = C
    assert _raw_call(ref_ctx, Q, n, 5, k, bad, C, **s.kw()) == E_INVALID and "ref_cls[20] = 3" in _message(ref_ctx)
    bad[20] = -1
    assert _raw_call(ref_ctx, Q, n, 5, k, bad, C, **s.kw()) == E_INVALID and "ref_cls[20] = -1" in _message(ref_ctx)
    assert _raw_call(ref_ctx, Q, n, 5, k, None, 0, **s.kw()) == E_INVALID and "needs ref_cls" in _message(ref_ctx)
    assert _raw_call(ref_ctx, Q, n, 5, k) == E_INVALID and "all outputs are null" in _message(ref_ctx)
    assert _raw_call(ref_ctx, None, n, 5, k, cls, C, **s.kw()) == E_INVALID and "(query): null matrix" in _message(ref_ctx)
    assert _raw_call(ref_ctx, Q, n, 5, k, cls, C, persp=7, **s.kw()) == E_INVALID and "perspective" in _message(ref_ctx)
    with pytest.raises(_lib.IciktError, match="exceeds the query_capacity"):
        ref_ctx.cross_prepared(wide, k)
    assert s.untouched()
    assert ref_ctx.reference_info() == (n, Sr, CAP)
    _check(ref_ctx, yard, Q, R, k, cls, C)              # and the next valid batch is still right

    # whatever replaces the prepared state drops the reference
    X = np.asfortranarray(np.hstack([Q, R]))
    for other in (lambda: ref_ctx.topk(X, 3), lambda: ref_ctx.pairs_complete(X, [0, 1], [2, 3]),
                  lambda: ref_ctx.cross(Q, R, k), lambda: ref_ctx.pairs(X)):
        ref_ctx.prepare_reference(R, CAP)
        assert ref_ctx.reference_info() == (n, Sr, CAP)
        other()
        assert _raw_call(ref_ctx, Q, n, 5, k, cls, C, **s.kw()) == E_STATE and "no prepared reference" in _message(ref_ctx)
        assert _lib.lib().icikt_ref_info(ref_ctx._h, None, None, None) == E_STATE
    assert s.untouched()
    ref_ctx.prepare_reference(R, CAP)
    _check(ref_ctx, yard, Q, R, k, cls, C)              # after a new prepare_reference it is right again
    # a second reference replaces the first
    Q2, R2 = _continuous(3, 6, 50)
    ref_ctx.prepare_reference(R2, 4)
    assert ref_ctx.reference_info() == (50, 6, 4)
    _check(ref_ctx, yard, Q2, R2, 2)


def test_block_cuts_give_identical_output(plan_ctx, yard):
    """tkblock=1: a query row per block, every row unpaired; 66: blocks of two rows and a trailing single row; 100:
    the same cut by a budget that is no multiple of the row; default: one block."""
    Sq, Sr, n, k, C = 5, 33, 40, 7, 4
    Q, R = _continuous(Sq, Sr, n)
    cls = (np.arange(Sr) * 7 % C).astype(np.int32)
    plan_ctx.prepare_reference(R, CAP)
    outs = []
    for spec in ("tkblock=1", "tkblock=66", "tkblock=100", None):
        plan_ctx.debug_set_plan(spec)
        outs.append(_check(plan_ctx, yard, Q, R, k, cls, C)[0])
    for got in outs:
        _same_results(got, outs[0])


@pytest.mark.parametrize("kind", ["tied", "continuous"])
def test_long_columns(ref_ctx, yard, kind):
    """15 000 rows: the range where the tie verdict is read back from the first prepared columns -- the reference's here,
    the query's in Context.cross -- and kept across the batches."""
    n, Sq, Sr = 15000, 3, 6
    rng = np.random.default_rng(41)
    X = rng.standard_normal((n, 2 * Sq + Sr))
    if kind == "tied":
        X = np.round(X * 40) / 40
        assert len(np.unique(X[:, 0])) <= 400
    X[rng.random(X.shape) < 0.02] = np.nan
    R = np.asfortranarray(X[:, 2 * Sq:])
    ref_ctx.prepare_reference(R, 4)
    _check(ref_ctx, yard, np.asfortranarray(X[:, :Sq]), R, 3)
    _check(ref_ctx, yard, np.asfortranarray(X[:, Sq:2 * Sq]), R, 3)


# ---- the class table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [None, "medlds=0"])
def test_class_table_on_the_signal_matrix(plan_ctx, yard, spec):
    """signal_matrix() split 30 / 100, the reference labelled by the matrix's own classes (of 1, 2, 3, 60 and 64 columns
    over both parts; class index 2 of the 6 is empty): even and odd cells, cells of one and two partners."""
    X, _labels, _names = signal_matrix()
    cls_all, C = interleaved()
    Q, R, cls = np.asfortranarray(X[:, :30]), np.asfortranarray(X[:, 30:]), np.ascontiguousarray(cls_all[30:])
    sizes = np.bincount(cls, minlength=C)
    assert sizes[2] == 0 and sizes.min() == 0 and 0 < sorted(sizes)[1] <= 3 and sizes.max() > 40
    plan_ctx.prepare_reference(R, 30)
    plan_ctx.debug_set_plan(spec)
    got, want = _check(plan_ctx, yard, Q, R, 5, cls, C)
    med2, n_valid = got[6], got[7]
    assert np.all(n_valid[:, 2] == 0) and np.all(bits(med2[:, :, 2]) == NA_REAL_BITS)
    assert np.all(n_valid[17] == 0)                                   # the constant query column has no partner at all
    assert {int(v) & 1 for v in n_valid[n_valid > 0]} == {0, 1}
    levels = [f"batch{c}" for c in range(C)]
    clear = clear_nearest(med2[1], n_valid)
    assert clear.sum() >= 25
    mine = api._nearest_class(med2[1], n_valid, levels)
    want2, want_n = brute_cross_class(want[0], cls, C)
    theirs = nearest(want2[1], want_n, levels)
    assert [a for a, ok in zip(mine, clear) if ok] == [b for b, ok in zip(theirs, clear) if ok]


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
    R[:, 8] = R[:, 4]            # a duplicate column: equal raw for every query
    R[:, 0] = Q[:, 0]            # a column in both matrices: a partner like any other
    return Q, R


@pytest.mark.parametrize("spec", [None, "medlds=0", "tkblock=1"])
def test_class_table_with_na_constant_and_duplicate_columns(plan_ctx, yard, spec):
    Q, R = _na_matrices()
    cls = np.array([0, 0, 3, 2, 2, 1, 3, 1, 2], dtype=np.int32)    # class 3: the constant and the all-missing column; 4: empty
    plan_ctx.prepare_reference(R, 4)
    plan_ctx.debug_set_plan(spec)
    got, _want = _check(plan_ctx, yard, Q, R, 9, cls, 5)
    med2, n_valid = got[6], got[7]
    assert n_valid.tolist() == [[2, 2, 3, 0, 0], [0] * 5, [2, 2, 3, 0, 0], [0] * 5]
    assert np.all(bits(med2[:, [1, 3]]) == NA_REAL_BITS) and np.all(bits(med2[:, :, 3:]) == NA_REAL_BITS)
    assert med2[1, 0, 0] > 0.2                                      # its own column is one of the two partners of (q0, c0)


@pytest.mark.parametrize("spec", [None, "medlds=0"])
def test_class_of_5000_members(plan_ctx, yard, spec):
    """Past the 4 096 keys of the LDS stage: every pass re-reads the records.  16 rows give tau a few hundred distinct
    values, so the select walks through long runs of equal keys; 5 037 reference columns: the padding column is there."""
    Sq, Sr, n = 2, 5037, 16
    Q, R = _continuous(Sq, Sr, n)
    cls = np.zeros(Sr, dtype=np.int32)
    cls[np.random.default_rng(2).choice(Sr, 37, replace=False)] = 1
    plan_ctx.prepare_reference(R, 2)
    plan_ctx.debug_set_plan(spec)
    got, want = _check(plan_ctx, yard, Q, R, 5, cls, 2)
    assert got[7][:, 0].min() > 4096
    raw_row = want[0][1][0]
    assert len(np.unique(raw_row[~np.isnan(raw_row)])) < 1000


def test_one_class_without_scaling(hip_ctx, yard):
    Q, R = _continuous(5, 65, 40)
    hip_ctx.prepare_reference(R, CAP)
    cls = np.zeros(65, dtype=np.int32)
    got, _want = _check(hip_ctx, yard, Q, R, 3, cls, 1, scale_max=False)
    assert np.array_equal(bits(got[6][0]), bits(got[6][1]))
    scaled, _want = _check(hip_ctx, yard, Q, R, 3, cls, 1)
    assert np.array_equal(bits(scaled[6][1]), bits(got[6][1]))      # med_raw does not depend on the scale


# ---- arguments -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [("global", True, "two.sided", False), ("local", True, "two.sided", False),
                                 ("global", False, "two.sided", False), ("local", False, "less", True),
                                 ("global", True, "greater", True)])
def test_arguments(hip_ctx, yard, cfg):
    """Both perspectives, scale_max on and off, a non-default alternative with continuity, and a global_na list with
    NaN, Inf, 0 and 5 that both matrices hold: recorded with the reference, applied to the batch."""
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
    cls = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
    hip_ctx.prepare_reference(R, 4, gna)
    got, _want = _check(hip_ctx, yard, Q, R, 4, cls, 2, gna, perspective, alternative, continuity, scale_max)
    hip_ctx.prepare_reference(R, 4)
    plain = hip_ctx.cross_prepared(Q, 4)
    assert not np.array_equal(bits(plain[0][1]), bits(got[0][1]))     # (the list changes the answer: it was applied)


def test_views_of_different_type_and_order(hip_ctx, yard):
    """A C-ordered float32 query against an F-ordered int32 reference, each read where it lies."""
    rng = np.random.default_rng(23)
    n, Sq, Sr, k = 40, 5, 12, 6
    Q32 = np.ascontiguousarray(rng.standard_normal((n, Sq)).astype(np.float32))
    Q32[rng.random((n, Sq)) < 0.08] = np.nan
    Ri = np.asfortranarray(rng.integers(-20, 20, size=(n, Sr)).astype(np.int32))
    assert _lib.input_view(Q32)[1:4] == (_lib.DTYPE_F32, _lib.ORDER_ROW, Sq)
    assert _lib.input_view(Ri)[1:5] == (_lib.DTYPE_I32, _lib.ORDER_COL, n, False)
    cls = (np.arange(Sr) % 2).astype(np.int32)
    hip_ctx.prepare_reference(Ri, CAP)
    got = hip_ctx.cross_prepared(Q32, k, True, cls, 2)
    Q64, R64 = np.asfortranarray(Q32, dtype=np.float64), np.asfortranarray(Ri, dtype=np.float64)
    want = yard.cross(Q64, R64, k)
    _same_results(got[:6], want)
    _assert_classes(got, want[0], cls, 2)


def test_f64_entries_match_the_view_entries(ref_ctx, yard):
    Q, R = _continuous(5, 65, 40)
    cls = (np.arange(65) % 4).astype(np.int32)
    ref_ctx.prepare_reference(R, CAP)
    want = ref_ctx.cross_prepared(Q, 7, True, cls, 4)
    ref_ctx.f64_entries = True
    try:
        ref_ctx.prepare_reference(R, CAP)
        got = ref_ctx.cross_prepared(Q, 7, True, cls, 4)
    finally:
        ref_ctx.f64_entries = False
    _same_results(got, want)
    _same_results(got[:6], yard.cross(Q, R, 7))


def test_output_subsets(hip_ctx, yard):
    Sq, Sr, n, k = 5, 65, 40, 7
    Q, R = _continuous(Sq, Sr, n)
    cls = (np.arange(Sr) % 3).astype(np.int32)
    want = yard.cross(Q, R, k)
    hip_ctx.prepare_reference(R, CAP)
    lists = hip_ctx.cross_prepared(Q, k, want_matrix=False)                 # top-k alone
    assert lists[0] is None and lists[6] is None and lists[7] is None
    _same_results(lists[1:6], want[1:])
    table = hip_ctx.cross_prepared(Q, None, False, cls, 3)                  # the class table alone
    assert table[0] is None and table[1] is None and table[2] is None and table[3] is None
    assert table[4] == want[4] and np.array_equal(table[5], want[5])
    _assert_classes(table, want[0], cls, 3)
    planes = hip_ctx.cross_prepared(Q)                                      # the matrices alone
    _same_results(planes[:1], want[:1])
    # cls_n_valid alone, through the C entry: every output is optional on its own
    cn = np.full((3, Sq), -9, dtype=np.int32)
    assert _raw_call(hip_ctx, Q, n, Sq, 0, cls, 3, cls_n=cn) == 0
    assert np.array_equal(cn.T, table[7])


def test_empty_query(hip_ctx, yard):
    Q, R = _continuous(3, 5, 40)
    cls = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    hip_ctx.prepare_reference(R, 4)
    got = hip_ctx.cross_prepared(Q[:, :0], 2, True, cls, 2)
    _same_results(got[:6], yard.cross(Q[:, :0], R, 2))
    assert got[6].shape == (2, 0, 2) and got[7].shape == (0, 2) and got[4] == -np.inf
    _check(hip_ctx, yard, Q, R, 2, cls, 2)             # the reference is still there


def test_on_a_caller_stream(yard):
    """One batch on a caller's side stream that is still busy: the entry may not return before the stream has reached
    it, and its result is the yardstick's."""
    import torch
    from tests.test_gpu_caller_stream import HOST_GATE_S, Gate, Lane
    X = sc.true_matrix(sc.Case(700, "continuous"))
    Q, R = np.asfortranarray(X[:, :3]), np.asfortranarray(X[:, 3:])
    cls = (np.arange(R.shape[1]) % 2).astype(np.int32)
    want = yard.cross(Q, R, 4)
    gate = Gate()
    ctx = _lib.Context(0)
    try:
        lane = Lane(ctx, "side")
        lane.warm(gate)
        ctx.prepare_reference(R, 4)
        with torch.cuda.stream(lane.ts):
            gate.run(gate.seconds(HOST_GATE_S))
            e_gate = torch.cuda.Event()
            e_gate.record()
            held = not e_gate.query()
        got = ctx.cross_prepared(Q, 4, True, cls, 2)
        assert held, "the gate was over before the call"
        assert e_gate.query(), "returned before the stream it was told to use had reached it"
        _same_results(got[:6], want)
        _assert_classes(got, want[0], cls, 2)
    finally:
        ctx.close()


# ---- the front end -------------------------------------------------------------------------------------------------
def test_front_end_matches_the_oracle_engine():
    from tests.oracle_engine import OracleEngine
    rng = np.random.default_rng(34)
    n, Sq, Sr, k = 300, 7, 9, 5
    X = rng.standard_normal((n, Sq + Sr))
    X[rng.random(X.shape) < 0.08] = np.nan
    X[X > 2.2] = 0.0                                   # zeros: missing under the default global_na
    Q, R = X[:, :Sq], X[:, Sq:]
    qn, rn = [f"q{i}" for i in range(Sq)], [f"r{j}" for j in range(Sr)]
    labels = list("aabbbccca")
    eng = api.HipEngine()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = api.ici_kendalltau_cross(Q, R, k=k, query_names=qn, reference_names=rn, reference_classes=labels,
                                        engine=OracleEngine())
        labelled = api.ici_kendalltau_cross(Q, R, k=k, query_names=qn, reference_names=rn, reference_classes=labels,
                                            engine=eng)
        with api.prepare_reference(R, 4, reference_names=rn, reference_classes=labels, engine=eng) as prepared:
            split = api.ici_kendalltau_cross(Q, prepared, k=k, query_names=qn)           # 4 + 3 columns
            again = api.ici_kendalltau_cross(Q[:, :2], prepared, k=k, query_names=qn[:2])
        with pytest.raises(ValueError, match="has been closed"):
            api.ici_kendalltau_cross(Q, prepared, k=k, query_names=qn)
        plain = api.ici_kendalltau_cross(Q, R, k=k, query_names=qn, reference_names=rn, engine=eng)
    assert "class_med_raw" not in plain and list(labelled) == list(want) == list(split)
    for got in (labelled, split):
        for key in ("indices", "n_valid", "neighbors", "class_n_valid", "class_levels", "nearest_class", "query_names",
                    "reference_names"):
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), key
        for name in list(KEYS) + ["topk_" + key for key in KEYS] + ["class_med_cor", "class_med_raw"]:
            a, b = np.asarray(got[name]), np.asarray(want[name])
            assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
            assert np.allclose(a, b, rtol=0, atol=1e-10, equal_nan=True), name      # (the oracle's tolerance, as for cross)
        assert abs(got["max_taumax"] - want["max_taumax"]) <= 1e-10
    # the labelled call is the plain call plus the tables, and the split call is the whole one in all that raw decides
    for key in plain:
        if key != "run_time":
            a, b = np.asarray(labelled[key]), np.asarray(plain[key])
            assert np.array_equal(bits(a), bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b), key
    for key in ("raw", "pvalue", "taumax", "completeness", "cor", "topk_raw", "topk_cor", "indices", "class_med_raw",
                "class_n_valid"):
        a, b = np.asarray(split[key]), np.asarray(labelled[key])
        assert np.array_equal(bits(a), bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b), key
    assert split["nearest_class"] == labelled["nearest_class"] and split["max_taumax"] == labelled["max_taumax"]
    assert np.array_equal(bits(again["raw"]), bits(np.asarray(labelled["raw"])[:2]))
