"""icikt_mst_f64 / _in / _csc on the GPU: the maximum spanning forest of the samples under raw, found by Boruvka rounds
over the kept plane.

The reference is the brute-force checker (tests/mst_checker.py: Kruskal in the strict edge order) applied to
Context.matrix over all pairs, computed once per data set: the edges and their order, the components and their
numbering, n_components, max_taumax and reason_counts must be EQUAL, the five value planes BITWISE equal to the
matrix's cells.  The shapes are the smallest that reach each part of the kernel: one edge, fewer partners than a wave, a
wave boundary, both read directions, a per-thread loop of several trips with a tail, equal keys that the tie-break
decides, several rounds, blocks of one row."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api, formats
from tests import designed_tau as dt
from tests.mst_checker import bits, brute_mst, tied_competitors, verify_forest
from tests.test_gpu_topk import _continuous, _edge_matrix

pytestmark = pytest.mark.gpu

_FULL = {}  # (data key, perspective, scale_max) -> (out5, max_taumax, reason_counts) of Context.matrix: computed once
_REF = {}   # (data key, perspective, scale_max, min_raw) -> (ti, tj, component, n_components)


def _full(ctx, key, X, global_na=None, perspective="global", scale_max=True):
    fk = (key, perspective, scale_max)
    if fk not in _FULL:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, perspective, "two.sided", False, 0, scale_max, True,
                                      want_keep=False)
        tm = out5[3][np.triu_indices(X.shape[1], k=1)]
        tm = tm[~np.isnan(tm)]
        _FULL[fk] = (out5, float(tm.max()) if tm.size else -np.inf, rc5)
    return _FULL[fk]


def _reference(ctx, key, X, min_raw=None, global_na=None, perspective="global", scale_max=True):
    full = _full(ctx, key, X, global_na, perspective, scale_max)
    rk = (key, perspective, scale_max, min_raw)
    if rk not in _REF:
        _REF[rk] = brute_mst(full[0][1], min_raw)
    return full, _REF[rk]


def _assert_same(got, ref):
    (out5, mx_ref, rc_ref), (ri, rj, rcomp, rn) = ref
    ti, tj, vals, component, n_comp, n_rounds, mx, rc5 = got
    S = out5.shape[1]
    print("S", S, "n_tree", len(ti), len(ri), "n_components", n_comp, rn, "n_rounds", n_rounds, "max_taumax", mx, mx_ref,
          "differing edges", int(np.sum((ti != ri) | (tj != rj))) if len(ti) == len(ri) else "length")
    assert ti.dtype == np.int32 and tj.dtype == np.int32 and component.dtype == np.int32
    assert len(ti) + n_comp == S
    assert np.array_equal(ti, ri) and np.array_equal(tj, rj)
    assert vals.shape == (5, len(ri))
    for q in range(5):
        assert np.array_equal(bits(vals[q]), bits(out5[q][ri, rj])), q
    assert np.array_equal(component, rcomp) and n_comp == rn
    assert mx == mx_ref
    assert np.array_equal(rc5, rc_ref)
    assert 0 <= n_rounds <= 17


def _same_bits(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
            and np.array_equal(a[3], b[3]) and a[4] == b[4] and a[6] == b[6] and np.array_equal(a[7], b[7]))


@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("S", [2, 3, 65, 130])
def test_small_shapes(hip_ctx, S, n):
    X = _continuous(S, n)
    ref = _reference(hip_ctx, ("cont", S, n), X)
    got = hip_ctx.mst(X)
    _assert_same(got, ref)
    assert got[4] == 1 and len(got[0]) == S - 1 and got[5] >= 1
    if S <= 130:
        verify_forest(ref[0][0][1], got[0], got[1], got[3])


@pytest.mark.parametrize("S", [300, 520])
def test_loop_with_a_tail(hip_ctx, S):
    X = _continuous(S, 40)
    _assert_same(hip_ctx.mst(X), _reference(hip_ctx, ("cont", S, 40), X))


@pytest.mark.parametrize("S", [1500, 1501])
def test_many_ties(hip_ctx, S):
    """16 rows (and the few counts of missing rows a pair can have) give tau a couple of thousand distinct values among
    1.1 million pairs, hundreds of pairs per value: equal keys decide edges, the tie-break is live, and one round does
    not finish the tree"""
    X = _continuous(S, 16)
    ref = _reference(hip_ctx, ("cont", S, 16), X)
    raw = ref[0][0][1]
    assert len(np.unique(raw[np.triu_indices(S, k=1)])) < 5000
    tied = tied_competitors(raw, ref[1][0], ref[1][1])
    print("tree edges with a tied competitor", tied, "of", S - 1)
    assert tied > (S - 1) // 2
    got = hip_ctx.mst(X)
    _assert_same(got, ref)
    assert got[5] >= 2


def test_identical_columns(hip_ctx):
    S, n = 130, 40
    col = np.random.default_rng(3).standard_normal(n)
    X = np.asfortranarray(np.tile(col[:, None], (1, S)))
    ref = _reference(hip_ctx, "same", X)
    got = hip_ctx.mst(X)
    _assert_same(got, ref)
    assert np.array_equal(got[0], np.zeros(S - 1)) and np.array_equal(got[1], np.arange(1, S))   # the star
    assert got[5] == 1 and len(set(bits(got[2][1]).tolist())) == 1


@pytest.mark.parametrize("cfg", [("global", True), ("local", True), ("global", False)])
def test_data_edge_cases(plan_ctx, cfg):
    """isolated samples (a constant and an all-missing column), three identical columns and their mirror image"""
    perspective, scale_max = cfg
    X = _edge_matrix()
    S = X.shape[1]
    ref = _reference(plan_ctx, "edge", X, None, None, perspective, scale_max)
    assert ref[1][3] >= 3 and ref[0][2][1:].sum() > 0
    assert np.sum(ref[1][2] == ref[1][2][3]) == 1 and np.sum(ref[1][2] == ref[1][2][7]) == 1
    for spec in (None, "tkblock=1"):
        plan_ctx.debug_set_plan(spec)
        got = plan_ctx.mst(X, None, None, perspective, "two.sided", False, 0, scale_max)
        _assert_same(got, ref)
        verify_forest(ref[0][0][1], got[0], got[1], got[3])
        if not scale_max:
            assert np.array_equal(bits(got[2][0]), bits(got[2][1]))


@pytest.mark.parametrize("which", ["p50", "p99", "above", "minus1"])
def test_min_raw(hip_ctx, which):
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    S, n = 130, 40
    X = _continuous(S, n)
    full = _full(hip_ctx, ("cont", S, n), X)
    tri = full[0][1][np.triu_indices(S, k=1)]
    t = {"p50": float(np.percentile(tri, 50)), "p99": float(np.percentile(tri, 99)), "above": float(tri.max()) + 0.125,
         "minus1": -1.0}[which]
    ref = _reference(hip_ctx, ("cont", S, n), X, t)
    got = hip_ctx.mst(X, t)
    _assert_same(got, ref)
    verify_forest(full[0][1], got[0], got[1], got[3], t)
    if which == "above":
        assert len(got[0]) == 0 and got[4] == S and np.array_equal(got[3], np.arange(S)) and got[5] in (0, 1)
    if which == "minus1":
        assert got[4] == 1
    if which == "p99":
        assert 1 < got[4] < S
    # the components of the network ici_kendalltau_edges returns at the same cut-off
    ei, ej, _vals, n_edges, _deg, _mx, _rc = hip_ctx.edges(X, min_raw=t, max_edges=S * (S - 1) // 2)
    assert n_edges == len(ei)
    graph = sp.coo_matrix((np.ones(len(ei)), (ei, ej)), shape=(S, S))
    n_cc, labels = csgraph.connected_components(graph, directed=False)
    assert n_cc == got[4] and np.array_equal(labels, got[3])
    # ... and of the uncut tree, cut afterwards
    whole = hip_ctx.mst(X)
    res = {"i": whole[0], "j": whole[1], "raw": whole[2][1], "component": whole[3], "n_components": whole[4]}
    assert np.array_equal(formats.mst_cut(res, t), got[3])


@pytest.mark.parametrize("case", ["130", "1500"])
def test_block_cuts(plan_ctx, case):
    """tkblock=1: a row per block; 3 and 1000: several rows; each identical to the uncut call"""
    S = int(case)
    n = 40 if S == 130 else 16
    X = _continuous(S, n)
    ref = _reference(plan_ctx, ("cont", S, n), X)
    cuts = ("tkblock=1", "tkblock=3", "tkblock=1000") if S == 130 else ("tkblock=200000",)
    outs = []
    for spec in (None,) + cuts:
        plan_ctx.debug_set_plan(spec)
        outs.append(plan_ctx.mst(X))
        _assert_same(outs[-1], ref)
    for got in outs[1:]:
        assert _same_bits(got, outs[0]) and got[5] == outs[0][5]


def test_closed_form_on_the_device(hip_ctx):
    """the swaps design with positive signs and distinct k: the tree is the path through the columns sorted by k,
    its edges ordered on the integers -- no matrix from the library involved"""
    S, n = 17, 40
    ks = np.random.default_rng(8).permutation(n // 2 + 1)[:S]
    d = dt.swaps(S, n, seed=1, params=ks, signs=np.ones(S, dtype=np.int32))
    by_k = np.argsort(ks)
    a, b = by_k[:-1], by_k[1:]
    i, j = np.minimum(a, b), np.maximum(a, b)
    gap = np.abs(ks[a] - ks[b])
    order = np.lexsort((i * (2 * S - i - 1) // 2 + (j - i - 1), gap))
    ti, tj, vals, component, n_comp, _n_rounds, mx, rc5 = hip_ctx.mst(d.X, None, [np.nan, np.inf, 0.0])
    want_raw = d.value(d.m - 2 * gap[order])
    assert np.array_equal(ti, i[order]) and np.array_equal(tj, j[order])
    assert np.array_equal(bits(vals[1]), bits(want_raw)) and np.array_equal(bits(vals[0]), bits(want_raw))
    assert np.all(vals[3] == 1.0) and np.all(vals[4] == 1.0) and mx == 1.0
    assert n_comp == 1 and np.all(component == 0) and np.array_equal(rc5, d.reason_counts())


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.mst(X64, *args)
    finally:
        ctx.f64_entries = False


def test_float32_row_major_view_matches_float64(hip_ctx):
    S, n = 65, 40
    rng = np.random.default_rng(21)
    X32 = np.ascontiguousarray(rng.standard_normal((n, S)).astype(np.float32))
    X32[rng.random((n, S)) < 0.08] = np.nan
    assert X32.flags.c_contiguous and _lib.input_view(X32)[2] == _lib.ORDER_ROW
    X64 = np.asfortranarray(X32, dtype=np.float64)
    want = _f64_entry(hip_ctx, X64)
    got = hip_ctx.mst(X32)
    assert _same_bits(got, want)
    _assert_same(got, _reference(hip_ctx, "f32", X64))


def test_scipy_csc_matches_dense(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    gna = [np.nan, np.inf, 0.0]
    want = _f64_entry(hip_ctx, X, None, gna)
    got = hip_ctx.mst(A, None, gna)
    assert _same_bits(got, want)
    _assert_same(got, _reference(hip_ctx, "csc", X, None, gna))


def test_refusals_leave_outputs_and_context_untouched(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.pairs(X)                                   # a prepared matrix and a pair list to keep
    L = _lib.lib()
    E_INVALID = -1
    big = np.zeros((1, 65536), order="F")

    def call(Xa, n_feat, n_samp, perspective, null=None):
        room = min(n_samp, 64)                         # (a refused call writes nothing: no room for what it cannot fill)
        ti = np.full(room, -7, dtype=np.int32)
        tj = np.full(room, -7, dtype=np.int32)
        vals = np.full((5, room), 123.25)
        comp = np.full(room, -7, dtype=np.int32)
        cells = {k: np.full(1, -9, dtype=np.int64) for k in ("n_tree", "n_components")}
        n_rounds = np.full(1, -9, dtype=np.int32)
        mx = np.full(1, 55.5)
        rc5 = np.full(5, -9, dtype=np.int64)
        outs = {"ti": ti, "tj": tj, "out5t": vals, "n_tree": cells["n_tree"], "component": comp,
                "n_components": cells["n_components"], "n_rounds": n_rounds}
        ptr = {k: (None if k == null else _lib._ptr(a)) for k, a in outs.items()}
        rc = L.icikt_mst_f64(hip_ctx._h, _lib._ptr(Xa), n_feat, n_samp, max(n_feat, 1), None, 0, perspective, 0, 0, 0, 1,
                             float("nan"), ptr["ti"], ptr["tj"], ptr["out5t"], ptr["n_tree"], ptr["component"],
                             ptr["n_components"], ptr["n_rounds"], _lib._ptr(mx), _lib._ptr(rc5))
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == E_INVALID, rc
        assert msg and msg.startswith(b"mst:"), msg
        assert np.all(ti == -7) and np.all(tj == -7) and np.all(vals == 123.25) and np.all(comp == -7)
        assert cells["n_tree"][0] == -9 and cells["n_components"][0] == -9 and n_rounds[0] == -9
        assert mx[0] == 55.5 and np.all(rc5 == -9)
        assert hip_ctx.num_pairs() == S * (S - 1) // 2    # the refused call touched nothing
        return msg.decode()

    msg = call(big, 1, 65536, 1)
    assert "ICIKT_TOPK_MAX_SAMPLES" in msg and "32 bits" in msg
    for name in ("ti", "tj", "out5t", "n_tree", "component", "n_components", "n_rounds"):
        assert f"null output ({name})" in call(X, n, S, 1, null=name)
    assert "perspective" in call(X, n, S, 7)
    with pytest.raises(_lib.IciktError, match="mst: perspective"):
        hip_ctx.mst(X, perspective="sideways")
    assert hip_ctx.num_pairs() == S * (S - 1) // 2
    out, _cnt, rsn = hip_ctx.pairs(X)                  # and the next ordinary call succeeds
    assert out.shape == (S * (S - 1) // 2, 4) and np.all(rsn == 0)


def test_state_after_a_successful_call(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    for min_raw in (None, 2.0):
        hip_ctx.pairs(X)
        ti, tj, vals, component, n_comp, n_rounds, mx, rc5 = hip_ctx.mst(X, min_raw)
        assert hip_ctx.num_pairs() == -1
        rc = _lib.lib().icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
        assert rc == -5, rc                            # ICIKT_E_STATE: nothing prepared
        assert len(ti) + n_comp == S and rc5.sum() == S * (S - 1) // 2 and np.isfinite(mx)
    assert n_comp == S and len(ti) == 0                # (the last call: no raw reaches 2)
    out, _cnt, _rsn = hip_ctx.pairs(X)
    assert out.shape[0] == S * (S - 1) // 2
    # slots behind n_tree stay untouched, and one sample is one component without an edge
    one = hip_ctx.mst(X[:, :1])
    assert len(one[0]) == 0 and one[4] == 1 and one[5] == 0 and np.array_equal(one[3], [0])


def test_front_end_matches_the_checker_engine(hip_ctx):
    """A designed matrix, where the HIP engine and the CPU oracle both give num / m exactly: the tree, its order, the
    components and the names are identical; the five values agree within 1e-10, the project's parity bound."""
    from tests.oracle_engine import OracleEngine
    S, n = 14, 40
    d = dt.swaps(S, n, seed=3, n_all_missing=1, n_constant=1)
    names = [f"s{i}" for i in range(S)]
    res, msgs = [], []
    for eng in (api.HipEngine(), OracleEngine()):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            res.append(api.ici_kendalltau_mst(d.X, colnames=names, engine=eng))
        msgs.append(sorted(str(x.message) for x in w if str(x.message) in _lib.REASON_WARNINGS.values()))
    got, want = res
    assert msgs[0] == msgs[1] and len(msgs[0]) == S - 2            # the constant column's pairs with a value column
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["j"], want["j"])
    assert list(got["s1"]) == list(want["s1"]) and list(got["s2"]) == list(want["s2"])
    assert list(got["sample_id"]) == list(want["sample_id"]) == names
    assert np.array_equal(got["component"], want["component"])
    assert got["n_components"] == want["n_components"] == 3 and got["n_tree"] == want["n_tree"] == S - 3
    for key in ("cor", "raw", "pvalue", "taumax", "completeness"):
        print(key, np.max(np.abs(got[key] - want[key])))
        assert got[key].shape == want[key].shape == (S - 3,)
        assert np.allclose(got[key], want[key], rtol=0, atol=1e-10), key
    assert abs(got["max_taumax"] - want["max_taumax"]) <= 1e-10
    bi, bj, bcomp, bn = brute_mst(d.raw)
    assert np.array_equal(got["i"], bi) and np.array_equal(got["j"], bj) and np.array_equal(got["component"], bcomp)
    assert np.array_equal(bits(got["raw"]), bits(d.raw[bi, bj]))
