"""icikt_topk_f64 / _in / _csc on the GPU: every sample's k best partners, selected on the device.

The reference is the brute-force checker (tests/topk_checker.py) applied to Context.matrix on the same input: idx and
n_valid must be equal and the five value planes BITWISE equal (the padding carries R's NA_real_ bits).  The shapes are
the smallest that reach each part of the selection kernel: one and several 256-wide passes over a column's candidates,
more than one sort round, full 256-entry lists, blocks of one row and blocks that end mid-triangle."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.topk_checker import NA_REAL_BITS, brute_topk, ranked_partners

pytestmark = pytest.mark.gpu

_REF = {}   # (data key, perspective, scale_max, alternative, continuity) -> (out5, ranked partners): computed once


def _continuous(S, n, seed=11):
    rng = np.random.default_rng(seed + 1000 * S + n)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X


def _reference(ctx, key, X, k, global_na=None, perspective="global", scale_max=True, alternative="two.sided",
               continuity=False):
    rk = (key, perspective, scale_max, alternative, continuity)
    if rk not in _REF:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, perspective, alternative, continuity, 0, scale_max, True,
                                      want_keep=False)
        _REF[rk] = (out5, ranked_partners(out5[1]), rc5)
    out5, ranked, rc5 = _REF[rk]
    return brute_topk(out5, k, ranked), out5, rc5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_same(got, ref):
    idx, vals, n_valid = got[0], got[1], got[2]
    ridx, rvals, rn = ref
    assert np.array_equal(n_valid, rn)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(_bits(vals), _bits(rvals))
    pad = idx < 0
    assert np.array_equal(pad, np.arange(idx.shape[1])[None, :] >= n_valid[:, None])
    for q in range(5):
        assert np.all(_bits(vals[q])[pad] == NA_REAL_BITS)


@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("S", [2, 3, 65, 130])
def test_small_shapes(hip_ctx, S, n):
    X = _continuous(S, n)
    k = min(7, S + 1)
    ref, out5, rc5 = _reference(hip_ctx, ("cont", S, n), X, k)
    got = hip_ctx.topk(X, k)
    _assert_same(got, ref)
    tm = out5[3][np.triu_indices(S, k=1)]
    assert got[3] == tm[~np.isnan(tm)].max()
    assert np.array_equal(got[4], rc5)


@pytest.mark.parametrize("k", ["1", "7", "S-1", "S+5"])
def test_k_edges(hip_ctx, k):
    S, n = 65, 40
    X = _continuous(S, n)
    k = {"1": 1, "7": 7, "S-1": S - 1, "S+5": S + 5}[k]
    ref, _out5, _rc = _reference(hip_ctx, ("cont", S, n), X, k)
    got = hip_ctx.topk(X, k)
    _assert_same(got, ref)
    assert np.array_equal(got[2], np.full(S, min(k, S - 1)))


def test_cap_full_lists(hip_ctx):
    S, n, k = 300, 50, 256
    X = _continuous(S, n)
    ref, _out5, _rc = _reference(hip_ctx, ("cont", S, n), X, k)
    _assert_same(hip_ctx.topk(X, k), ref)


@pytest.mark.parametrize("k", [5, 100])
def test_many_candidates_and_index_ties(hip_ctx, k):
    """1 499 candidates per column: several 256-wide passes and more than one sort round; 16 rows give tau a few hundred
    distinct values at most (121 without missing cells), so every column has partners of equal raw among its 1 499
    and the index decides."""
    S, n = 1500, 16
    X = _continuous(S, n)
    ref, out5, _rc = _reference(hip_ctx, ("cont", S, n), X, k)
    raw_row = out5[1][0][1:]
    assert len(np.unique(raw_row[~np.isnan(raw_row)])) < 1000      # (the ties the case is about are there)
    _assert_same(hip_ctx.topk(X, k), ref)


def test_block_cuts_give_identical_output(plan_ctx):
    S, n, k = 130, 40, 7
    X = _continuous(S, n)
    ref, _out5, rc5 = _reference(plan_ctx, ("cont", S, n), X, k)
    outs = []
    for spec in ("tkblock=1", "tkblock=1000", None):
        plan_ctx.debug_set_plan(spec)
        outs.append(plan_ctx.topk(X, k))
    for got in outs:
        _assert_same(got, ref)
        assert got[3] == outs[0][3]
        assert np.array_equal(got[4], rc5)


def test_blocks_at_the_cap(plan_ctx):
    """Full lists carried from block to block: k = 256 at S = 300, a row per block and blocks of a few rows."""
    S, n, k = 300, 50, 256
    X = _continuous(S, n)
    ref, _out5, _rc = _reference(plan_ctx, ("cont", S, n), X, k)
    for spec in ("tkblock=1", "tkblock=2500"):
        plan_ctx.debug_set_plan(spec)
        _assert_same(plan_ctx.topk(X, k), ref)


def _edge_matrix():
    rng = np.random.default_rng(5)
    n, S = 40, 12
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    X[:, 4] = X[:, 1]
    X[:, 9] = X[:, 1]            # three identical columns
    X[:, 6] = -X[:, 1]           # and their mirror image
    X[:, 3] = 1.25               # constant: reason 3 with every partner
    X[:, 7] = np.nan             # all missing
    X[:, 10] = np.nan
    X[17, 10] = 0.5              # a single non-missing row
    return X


@pytest.mark.parametrize("cfg", [("global", True, "two.sided", False), ("local", True, "two.sided", False),
                                 ("global", False, "two.sided", False), ("global", True, "less", False),
                                 ("global", True, "two.sided", True)])
def test_data_edge_cases(plan_ctx, cfg):
    perspective, scale_max, alternative, continuity = cfg
    X = _edge_matrix()
    S = X.shape[1]
    ref, out5, rc5 = _reference(plan_ctx, "edge", X, S - 1, None, perspective, scale_max, alternative, continuity)
    for spec in (None, "tkblock=1"):
        plan_ctx.debug_set_plan(spec)
        got = plan_ctx.topk(X, S - 1, None, perspective, alternative, continuity, 0, scale_max)
        _assert_same(got, ref)
        assert np.array_equal(got[4], rc5)
    idx, n_valid = got[0], got[2]
    assert n_valid[3] == 0 and n_valid[7] == 0 and not np.any(np.isin(idx, (3, 7)))
    if perspective == "global":
        row = idx[0].tolist()
        at = [row.index(j) for j in (1, 4, 9)]
        assert at == [at[0], at[0] + 1, at[0] + 2]                 # equal raw: by index
        assert idx[1, :2].tolist() == [4, 9] and idx[9, :2].tolist() == [1, 4]


def test_float32_row_major_view_matches_float64(hip_ctx):
    S, n, k = 65, 40, 9
    rng = np.random.default_rng(21)
    X32 = np.ascontiguousarray(rng.standard_normal((n, S)).astype(np.float32))
    X32[rng.random((n, S)) < 0.08] = np.nan
    assert X32.flags.c_contiguous and _lib.input_view(X32)[2] == _lib.ORDER_ROW
    X64 = np.asfortranarray(X32, dtype=np.float64)
    want = hip_ctx.topk(X64, k)
    got = hip_ctx.topk(X32, k)
    _assert_same(got, want[:3])
    assert got[3] == want[3] and np.array_equal(got[4], want[4])
    ref, _out5, _rc = _reference(hip_ctx, "f32", X64, k)
    _assert_same(got, ref)


def test_csc_view_matches_dense(hip_ctx):
    S, n, k = 65, 40, 9
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    rows, cols = np.nonzero(X.T)[1], np.nonzero(X.T)[0]
    indptr = np.concatenate([[0], np.cumsum((X != 0).sum(axis=0))]).astype(np.int32)
    view = _lib.CscView(np.ascontiguousarray(X.T[X.T != 0]), rows.astype(np.int32), indptr, (n, S), 0.0, False)
    assert np.array_equal(view.toarray(), X)
    gna = [np.nan, np.inf, 0.0]
    want = hip_ctx.topk(X, k, gna)
    got = hip_ctx.topk(view, k, gna)
    _assert_same(got, want[:3])
    assert got[3] == want[3] and np.array_equal(got[4], want[4])
    ref, _out5, _rc = _reference(hip_ctx, "csc", X, k, gna)
    _assert_same(got, ref)


def test_argument_errors_leave_the_context_usable(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.pairs(X)                                   # a prepared matrix and a pair list to keep
    for k in (0, 257):
        with pytest.raises(_lib.IciktError, match=r"topk: k must be in 1 \.\. ICIKT_TOPK_MAX"):
            hip_ctx.topk(X, k)
    with pytest.raises(_lib.IciktError, match="topk: perspective"):
        hip_ctx.topk(X, 3, perspective="sideways")
    L = _lib.lib()
    idx = np.empty((S, 3), dtype=np.int32)
    vals = np.empty((5, S, 3), dtype=np.float64)
    for name, a_idx, a_vals in (("idx", None, vals), ("out5k", idx, None)):
        rc = L.icikt_topk_f64(hip_ctx._h, _lib._ptr(X), n, S, n, None, 0, 3, 1, 0, 0, 0, 1, _lib._ptr(a_idx),
                              _lib._ptr(a_vals), None, None, None)
        with pytest.raises(_lib.IciktError, match=rf"null output \({name}\)"):
            hip_ctx._chk(rc, "icikt_topk_f64")
    rc = L.icikt_topk_f64(hip_ctx._h, None, n, S, n, None, 0, 3, 1, 0, 0, 0, 1, _lib._ptr(idx), _lib._ptr(vals), None,
                          None, None)
    with pytest.raises(_lib.IciktError, match="topk: null matrix"):
        hip_ctx._chk(rc, "icikt_topk_f64")
    assert hip_ctx.num_pairs() == S * (S - 1) // 2    # refused calls touched nothing
    out, _cnt, rsn = hip_ctx.pairs(X)                  # and the next ordinary call succeeds
    assert out.shape == (S * (S - 1) // 2, 4) and np.all(rsn == 0)


def test_state_after_a_successful_call(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.topk(X, 3)
    assert hip_ctx.num_pairs() == -1
    rc = _lib.lib().icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
    assert rc == -5, rc                                # ICIKT_E_STATE: nothing prepared
    out, _cnt, _rsn = hip_ctx.pairs(X)
    assert out.shape[0] == S * (S - 1) // 2


def test_too_many_samples_is_refused(hip_ctx):
    X = np.zeros((1, 65536), order="F")
    with pytest.raises(_lib.IciktError, match="ICIKT_TOPK_MAX_SAMPLES"):
        hip_ctx.topk(X, 1)


def test_front_end_matches_the_oracle_engine(hip_ctx):
    from tests.oracle_engine import OracleEngine
    S, n, k = 12, 300, 5
    rng = np.random.default_rng(33)
    X = rng.standard_normal((n, S))
    X[rng.random((n, S)) < 0.08] = np.nan
    X[X > 2.2] = 0.0                                   # zeros: missing under the default global_na
    names = [f"s{i}" for i in range(S)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = api.ici_kendalltau_topk(X, k, colnames=names, engine=api.HipEngine())
        want = api.ici_kendalltau_topk(X, k, colnames=names, engine=OracleEngine())
    assert np.array_equal(got["indices"], want["indices"])
    assert np.array_equal(got["n_valid"], want["n_valid"])
    assert np.array_equal(got["neighbors"], want["neighbors"])
    for key in ("cor", "raw", "pvalue", "taumax", "completeness"):
        print(key, np.nanmax(np.abs(got[key] - want[key])))
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key]))
        assert np.allclose(got[key], want[key], rtol=0, atol=1e-10, equal_nan=True), key
    assert abs(got["max_taumax"] - want["max_taumax"]) <= 1e-10
