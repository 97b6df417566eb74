"""icikt_hclust_f64 / _in / _csc on the GPU: complete, average and single linkage of the samples under raw, run as
S - 1 steps of three launches over an S x S table of keys.

The reference is the brute-force checker (tests/hclust_checker.py: the rule as a naive loop in Python floats) applied to
Context.matrix of the same call arguments, computed once per data set: every integer must be EQUAL, every double BITWISE
equal, for all three methods.  The shapes are the smallest that reach each part of the kernels: one merge, fewer slots
than a wave, a wave and a workgroup boundary in pick and rescan, a merge grid with a tail, a rescan list longer than
the grid, equal keys that the tie-break decides at nearly every step, pairs without a raw."""
import ctypes

import numpy as np
import pytest

from icikendalltau_amd import _lib, api, formats
from tests.call_schedule import _csc
from tests.hclust_checker import METHODS, bits, brute_hclust
from tests.test_gpu_topk import _continuous, _edge_matrix

pytestmark = pytest.mark.gpu

_FULL = {}  # (data key, perspective, scale_max) -> (out5, max_taumax, reason_counts) of Context.matrix: computed once
_REF = {}   # (data key, perspective, scale_max, method, min_raw) -> brute_hclust's tuple


def _full(ctx, key, X, global_na=None, perspective="global", scale_max=True):
    fk = (key, perspective, scale_max)
    if fk not in _FULL:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, perspective, "two.sided", False, 0, scale_max, True,
                                      want_keep=False)
        tm = out5[3][np.triu_indices(X.shape[1], k=1)]
        tm = tm[~np.isnan(tm)]
        _FULL[fk] = (out5, float(tm.max()) if tm.size else -np.inf, rc5)
    return _FULL[fk]


def _reference(ctx, key, X, method, min_raw=None, global_na=None, perspective="global", scale_max=True):
    full = _full(ctx, key, X, global_na, perspective, scale_max)
    rk = (key, perspective, scale_max, method, min_raw)
    if rk not in _REF:
        _REF[rk] = brute_hclust(full[0][1], method, min_raw)
    return full, _REF[rk], scale_max


def _assert_same(got, ref):
    (out5, mx_ref, rc_ref), (ra, rb, rsize, rraw, rcomp, rn), scale_max = ref
    ma, mb, msize, mraw, mcor, component, n_comp, mx, rc5 = got
    S = out5.shape[1]
    same_len = len(ma) == len(ra)
    print("S", S, "n_merges", len(ma), len(ra), "n_components", n_comp, rn, "max_taumax", mx, mx_ref,
          "differing merges", int(np.sum((ma != ra) | (mb != rb))) if same_len else "length",
          "differing raw", int(np.sum(bits(mraw) != bits(rraw))) if same_len else "length")
    assert ma.dtype == np.int32 and mb.dtype == np.int32 and msize.dtype == np.int32 and component.dtype == np.int32
    assert len(ma) + n_comp == S
    assert np.array_equal(ma, ra) and np.array_equal(mb, rb) and np.array_equal(msize, rsize)
    assert np.array_equal(bits(mraw), bits(rraw))
    assert np.array_equal(bits(mcor), bits(rraw / mx_ref if scale_max else rraw))
    assert np.array_equal(component, rcomp) and n_comp == rn
    assert mx == mx_ref
    assert np.array_equal(rc5, rc_ref)


def _same_bits(a, b):
    return (all(np.array_equal(a[q], b[q]) for q in (0, 1, 2, 5)) and np.array_equal(bits(a[3]), bits(b[3]))
            and np.array_equal(bits(a[4]), bits(b[4])) and a[6] == b[6] and a[7] == b[7] and np.array_equal(a[8], b[8]))


@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("S", [2, 3, 65, 130])
def test_small_shapes(hip_ctx, S, n):
    X = _continuous(S, n)
    for method in METHODS:
        got = hip_ctx.hclust(X, method)
        _assert_same(got, _reference(hip_ctx, ("cont", S, n), X, method))
        assert got[6] == 1 and len(got[0]) == S - 1 and got[2][-1] == S


@pytest.mark.parametrize("S", [257, 520])
def test_tails(plan_ctx, S):
    """the merge grid has a workgroup with a tail; with hcgrid=1 one workgroup walks the whole rescan list"""
    X = _continuous(S, 40)
    for spec in (None, "hcgrid=1"):
        plan_ctx.debug_set_plan(spec)
        for method in METHODS:
            _assert_same(plan_ctx.hclust(X, method), _reference(plan_ctx, ("cont", S, 40), X, method))


def test_many_ties(plan_ctx):
    """8 rows (and the few counts of missing rows a pair can have) give tau on the order of a hundred values among
    44 850 pairs, hundreds of pairs per value: the tie-break decides nearly every step, and a neighbour that is not
    rescanned must still be the row's best in the strict order"""
    S, n = 300, 8
    X = _continuous(S, n)
    raw = _full(plan_ctx, ("cont", S, n), X)[0][1]
    tri = raw[np.triu_indices(S, k=1)]
    distinct = len(np.unique(tri[~np.isnan(tri)]))
    print("distinct raw values", distinct, "among", len(tri), "pairs")
    assert 100 * distinct < len(tri)
    for spec in (None, "hcgrid=7"):
        plan_ctx.debug_set_plan(spec)
        for method in METHODS:
            _assert_same(plan_ctx.hclust(X, method), _reference(plan_ctx, ("cont", S, n), X, method))


def test_identical_columns(hip_ctx):
    """all similarities equal: every step merges slot 1, 2, .. into slot 0"""
    S, n = 130, 40
    col = np.random.default_rng(3).standard_normal(n)
    X = np.asfortranarray(np.tile(col[:, None], (1, S)))
    for method in METHODS:
        got = hip_ctx.hclust(X, method)
        _assert_same(got, _reference(hip_ctx, "same", X, method))
        assert np.array_equal(got[0], np.zeros(S - 1)) and np.array_equal(got[1], np.arange(1, S))
        assert np.array_equal(got[2], np.arange(2, S + 1)) and len(set(bits(got[3]).tolist())) == 1


@pytest.mark.parametrize("cfg", [("global", True), ("local", True), ("global", False)])
def test_data_edge_cases(plan_ctx, cfg):
    """singleton components (a constant and an all-missing column), three identical columns and their mirror image"""
    perspective, scale_max = cfg
    X = _edge_matrix()
    S = X.shape[1]
    for method in METHODS:
        ref = _reference(plan_ctx, "edge", X, method, None, None, perspective, scale_max)
        comp = ref[1][4]
        assert ref[1][5] >= 3 and np.sum(comp == comp[3]) == 1 and np.sum(comp == comp[7]) == 1
        for spec in (None, "tkblock=1"):
            plan_ctx.debug_set_plan(spec)
            got = plan_ctx.hclust(X, method, None, None, perspective, "two.sided", False, 0, scale_max)
            _assert_same(got, ref)
            assert len(got[0]) + got[6] == S
            if not scale_max:
                assert np.array_equal(bits(got[3]), bits(got[4]))


@pytest.mark.parametrize("which", ["p50", "p99", "above", "minus1"])
def test_min_raw(hip_ctx, which):
    S, n = 130, 40
    X = _continuous(S, n)
    tri = _full(hip_ctx, ("cont", S, n), X)[0][1][np.triu_indices(S, k=1)]
    t = {"p50": float(np.percentile(tri, 50)), "p99": float(np.percentile(tri, 99)), "above": float(tri.max()) + 0.125,
         "minus1": -1.0}[which]
    for method in METHODS:
        got = hip_ctx.hclust(X, method, t)
        _assert_same(got, _reference(hip_ctx, ("cont", S, n), X, method, t))
        if which == "above":
            assert len(got[0]) == 0 and got[6] == S and np.array_equal(got[5], np.arange(S))
        if which == "minus1":
            assert got[6] == 1
        if which == "p99":
            assert 1 < got[6] < S
        whole = hip_ctx.hclust(X, method)
        res = {"merge_a": whole[0], "merge_b": whole[1], "raw": whole[3], "component": whole[5]}
        assert np.array_equal(formats.hclust_cut(res, t), got[5])
        m = len(got[0])
        assert _same_bits(tuple(w[:m] for w in whole[:5]) + got[5:], got)     # a stopped run is a prefix of the whole


@pytest.mark.parametrize("n", [8, 40])
def test_geometry(plan_ctx, n):
    """the block cut and the rescan grid change nothing"""
    S = 130
    X = _continuous(S, n)
    for method in METHODS:
        ref = _reference(plan_ctx, ("cont", S, n), X, method)
        outs = []
        for tk in (None, 1000, 1):
            for hg in (1, 7, None):
                plan_ctx.debug_set_plan({"tkblock": tk, "hcgrid": hg})
                outs.append(plan_ctx.hclust(X, method))
        _assert_same(outs[0], ref)
        for got in outs[1:]:
            assert _same_bits(got, outs[0])


def test_single_linkage_is_the_spanning_tree(hip_ctx):
    """distinct similarities: single linkage merges along the maximum spanning tree's edges in Kruskal's order.  (tau is
    a ratio of integers: 700 rows leave a handful of equal values among 8 385 pairs, so the shape is 780 pairs of 2 000
    rows, whose closest two values the CPU oracle puts 9.5e-8 apart.)"""
    S, n = 40, 2000
    X = _continuous(S, n, seed=12)
    tri = _full(hip_ctx, ("cont12", S, n), X)[0][1][np.triu_indices(S, k=1)]
    assert not np.any(np.isnan(tri)) and len(np.unique(tri)) == len(tri)
    got = hip_ctx.hclust(X, "single")
    ti, tj, vals, component, n_comp, _rounds, mx, rc5 = hip_ctx.mst(X)
    assert len(got[0]) == len(ti) == S - 1
    assert np.array_equal(bits(got[3]), bits(vals[1])) and np.array_equal(bits(got[4]), bits(vals[0]))
    assert got[7] == mx and np.array_equal(got[8], rc5) and np.array_equal(got[5], component)


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.hclust(X64, *args)
    finally:
        ctx.f64_entries = False


def test_float32_row_major_view_matches_float64(hip_ctx):
    S, n = 65, 40
    rng = np.random.default_rng(21)
    X32 = np.ascontiguousarray(rng.standard_normal((n, S)).astype(np.float32))
    X32[rng.random((n, S)) < 0.08] = np.nan
    assert X32.flags.c_contiguous and _lib.input_view(X32)[2] == _lib.ORDER_ROW
    X64 = np.asfortranarray(X32, dtype=np.float64)
    for method in METHODS:
        want = _f64_entry(hip_ctx, X64, method)
        got = hip_ctx.hclust(X32, method)
        assert _same_bits(got, want)
        _assert_same(got, _reference(hip_ctx, "f32", X64, method))


def test_scipy_csc_matches_dense(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    gna = [np.nan, np.inf, 0.0]
    for method in METHODS:
        want = _f64_entry(hip_ctx, X, method, None, gna)
        got = hip_ctx.hclust(A, method, None, gna)
        assert _same_bits(got, want)
        _assert_same(got, _reference(hip_ctx, "csc", X, method, None, gna))


def test_used_context():
    """One context serves a larger matrix, a smaller one, other data of the same shape, a refused call, the largest and
    the smallest, with alternating methods: every answer is the one a context created for the call gives, and the
    checker's.  A buffer that a call read beyond what it wrote -- the table's tail, a live flag, the list counter --
    would show here."""
    used = _lib.Context(0)
    try:
        calls = [(_continuous(130, 40), "complete", None), (_continuous(65, 40), "average", None),
                 (_continuous(65, 40, seed=12), "single", None), None, (_continuous(300, 8), "average", None),
                 (_continuous(3, 40), "complete", None), (_continuous(130, 8), "single", 0.0),
                 (_continuous(65, 40), "complete", None)]
        for k, call in enumerate(calls):
            if call is None:
                with pytest.raises(_lib.IciktError, match="hclust: method"):
                    used.hclust(_continuous(65, 40), "ward")
                continue
            X, method, min_raw = call
            got = used.hclust(X, method, min_raw)
            fresh = _lib.Context(0)
            try:
                want = fresh.hclust(X, method, min_raw)
                assert _same_bits(got, want), k
                _assert_same(got, _reference(fresh, ("used", k), X, method, min_raw))
            finally:
                fresh.close()
    finally:
        used.close()


def _raw_call(ctx, X, method=0, perspective=1, null=None):
    """the entry called on sentinel-filled outputs: (return code, message, the outputs)"""
    fn, _fname, xargs, _n_feat, n_samp, flags, _keep = ctx._entry("hclust", X, 0)
    room = min(max(n_samp - 1, 1), 512)               # (a refused call writes nothing: no room for what it cannot fill)
    outs = {"ma": np.full(room, -7, dtype=np.int32), "mb": np.full(room, -7, dtype=np.int32),
            "msize": np.full(room, -7, dtype=np.int32), "mraw": np.full(room, 123.25), "mcor": np.full(room, 123.25),
            "n_merges": np.full(1, -9, dtype=np.int64), "component": np.full(room + 1, -7, dtype=np.int32),
            "n_components": np.full(1, -9, dtype=np.int64)}
    mx = np.full(1, 55.5)
    rc5 = np.full(5, -9, dtype=np.int64)
    ptr = {k: (None if k == null else _lib._ptr(a)) for k, a in outs.items()}
    rc = fn(ctx._h, *xargs, None, 0, perspective, 0, 0, flags, 1, method, float("nan"), ptr["ma"], ptr["mb"],
            ptr["msize"], ptr["mraw"], ptr["mcor"], ptr["n_merges"], ptr["component"], ptr["n_components"], _lib._ptr(mx),
            _lib._ptr(rc5))
    outs["max_taumax"], outs["reason_counts"] = mx, rc5
    return rc, (_lib.lib().icikt_last_error(ctx._h) or b"").decode(), outs


def _arrays_untouched(outs):
    return (all(np.all(outs[k] == -7) for k in ("ma", "mb", "msize", "component"))
            and np.all(outs["mraw"] == 123.25) and np.all(outs["mcor"] == 123.25))


def test_refusals_leave_outputs_and_context_untouched(plan_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    plan_ctx.pairs(X)                                  # a prepared matrix and a pair list to keep
    E_INVALID = -1

    def refused(Xa, **kw):
        rc, msg, outs = _raw_call(plan_ctx, Xa, **kw)
        assert rc == E_INVALID and msg.startswith("hclust:"), (rc, msg)
        assert _arrays_untouched(outs)
        assert outs["n_merges"][0] == -9 and outs["n_components"][0] == -9
        assert outs["max_taumax"][0] == 55.5 and np.all(outs["reason_counts"] == -9)
        assert plan_ctx.num_pairs() == S * (S - 1) // 2    # the refused call touched nothing
        return msg

    for method in (3, -1, 17):
        assert "method must be complete (0), average (1) or single (2)" in refused(X, method=method)
    msg = refused(np.zeros((1, 65536), order="F"))
    assert "ICIKT_TOPK_MAX_SAMPLES" in msg
    for name in ("ma", "mb", "msize", "mraw", "mcor", "n_merges", "component", "n_components"):
        assert f"null output ({name})" in refused(X, null=name)
    assert "perspective" in refused(X, perspective=7)
    with pytest.raises(_lib.IciktError, match="hclust: method"):
        plan_ctx.hclust(X, "centroid")
    assert plan_ctx.num_pairs() == S * (S - 1) // 2
    out, _cnt, rsn = plan_ctx.pairs(X)                 # and the next ordinary call succeeds
    assert out.shape == (S * (S - 1) // 2, 4) and np.all(rsn == 0)
    # a duplicate CSC entry that the device finds while the matrix of a call of several blocks is uploaded: the call
    # fails, no merge is written, and the next call on the context is right
    X130 = _continuous(130, 40)
    plan_ctx.debug_set_plan("tkblock=1000")
    rc, msg, outs = _raw_call(plan_ctx, _csc(X130, dup_col=120))
    assert rc == E_INVALID and "duplicate entry" in msg, (rc, msg)
    assert _arrays_untouched(outs)
    for method in METHODS:
        _assert_same(plan_ctx.hclust(_csc(X130), method), _reference(plan_ctx, ("cont", 130, 40), X130, method))


def test_state_after_a_successful_call(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.pairs(X)
    got = hip_ctx.hclust(X)
    assert hip_ctx.num_pairs() == -1
    rc = _lib.lib().icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
    assert rc == -5, rc                                # ICIKT_E_STATE: nothing prepared
    assert len(got[0]) + got[6] == S and got[8].sum() == S * (S - 1) // 2
    one = hip_ctx.hclust(X[:, :1])                     # one sample is one cluster without a merge
    assert len(one[0]) == 0 and one[6] == 1 and np.array_equal(one[5], [0])
    rc, msg, outs = _raw_call(hip_ctx, X, method=1)    # slots behind n_merges stay untouched
    m = int(outs["n_merges"][0])
    assert rc == 0 and m == S - 1 and np.all(outs["ma"][m:] == -7) and np.all(outs["mraw"][m:] == 123.25)
    assert np.all(outs["component"][S:] == -7)


class _WithoutHclust:
    """the HIP engine as an engine that has no hclust method: the front end then goes through the full matrices"""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        if name == "hclust":
            raise AttributeError(name)
        return getattr(self._eng, name)


def test_front_end_matches_the_numpy_route(hip_ctx):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    S, n = 40, 30
    X = _continuous(S, n)
    names = [f"s{i}" for i in range(S)]
    eng = api.HipEngine()
    for method in METHODS:
        got = api.ici_kendalltau_hclust(X, method=method, colnames=names, engine=eng)
        want = api.ici_kendalltau_hclust(X, method=method, colnames=names, engine=_WithoutHclust(eng))
        for key in ("merge_a", "merge_b", "size", "component"):
            assert np.array_equal(got[key], want[key]) and got[key].dtype == np.int32, key
        for key in ("raw", "cor"):
            assert np.array_equal(bits(got[key]), bits(want[key])), key
        assert got["n_merges"] == want["n_merges"] == S - 1 and got["n_components"] == want["n_components"] == 1
        assert got["max_taumax"] == want["max_taumax"] and list(got["sample_id"]) == names and got["method"] == method
        Z = formats.hclust_to_linkage(got)             # the device result as scipy takes it
        assert hier.is_valid_linkage(Z, throw=True) and len(hier.leaves_list(Z)) == S
        assert np.array_equal(bits(Z[:, 2]), bits(1.0 - got["raw"]))
