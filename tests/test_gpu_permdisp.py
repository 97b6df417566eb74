"""icikt_permdisp_f64 / _in / _csc on the GPU: PERMDISP's fixed-point table, every sample's sum of squared
dissimilarities to every class, and the front end's distances to the class centroids.

The reference is the brute-force checker (tests/permdisp_checker.py: plain loops, Python ints, Fractions and 120-digit
decimal square roots) applied to the raw plane of Context.matrix over all pairs, computed once per data set and
labelling.  Every integer must be EQUAL (the values and NA pairs, Q, every cell of the table with the limbs combined,
reason_counts), max_taumax equal, and every double of the front end BITWISE equal.  The shapes are the smallest that
reach each part: one pair; a workgroup's stride of 256 partners, its edge (257) and past it (300); bins in LDS and in
global memory (2 049 declared classes); waves whose partners all share a class and waves that mix classes."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.permdisp_checker import bits, brute_permdisp, brute_table, documented_permutations, na_real
from tests.test_gpu_medians import _continuous
from tests.test_gpu_permanova import _balanced, _unequal5
from tests.test_gpu_quantiles import _few_rows
from tests.test_gpu_topk import _edge_matrix

pytestmark = pytest.mark.gpu

_FULL = {}  # data key -> (raw [S, S], max_taumax, reason_counts) of Context.matrix: computed once
_REF = {}   # (data key, labels key) -> brute_table's tuple


def _full(ctx, key, X, global_na=None):
    if key not in _FULL:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, "global", "two.sided", False, 0, True, True, want_keep=False)
        tm = out5[3][np.triu_indices(X.shape[1], k=1)]
        tm = tm[~np.isnan(tm)]
        _FULL[key] = (np.array(out5[1]), float(tm.max()) if tm.size else -np.inf, rc5)
    return _FULL[key]


def _reference(ctx, key, X, cls, n_class, lkey, global_na=None):
    full = _full(ctx, key, X, global_na)
    if (key, lkey) not in _REF:
        _REF[(key, lkey)] = brute_table(full[0], cls, n_class)
    return full, _REF[(key, lkey)]


def _assert_same(got, ref):
    (_raw, mx_ref, rc_ref), (n_val, n_na, Q_ref, T_ref, _A, _sizes) = ref
    n_pairs, Q, T, mx, rc5 = got
    want = np.array(T_ref, dtype=object).reshape(T.shape)
    print("values, n_na", list(n_pairs), [n_val, n_na], "Q", Q, Q_ref, "cells", T.size, "differing cells",
          int(np.sum(T != want)))
    assert n_pairs.dtype == np.int64 and list(n_pairs) == [n_val, n_na]
    assert isinstance(Q, int) and Q == Q_ref
    assert T.dtype == object and all(isinstance(v, int) for v in T.ravel())
    assert T.tolist() == T_ref
    assert mx == mx_ref and np.array_equal(rc5, rc_ref)


def _run(ctx, key, X, cls, n_class, lkey, global_na=None, **kw):
    ref = _reference(ctx, key, X, cls, n_class, lkey, global_na)
    got = ctx.permdisp(X, cls, n_class, global_na, **kw)
    _assert_same(got, ref)
    return got, ref


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2].tolist() == b[2].tolist() and a[3] == b[3]
            and np.array_equal(a[4], b[4]))


@pytest.mark.parametrize("S,n", [(2, 40), (3, 40), (65, 40), (130, 40), (257, 40), (300, 40), (130, 700)])
def test_shapes(hip_ctx, S, n):
    X = _continuous(S, n)
    cls, n_class = _balanced(S)
    got, _ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, "bal")
    assert got[0][0] == S * (S - 1) // 2 and got[0][1] == 0 and got[2].shape == (S, 2)
    assert sum(int(v) for v in got[2].ravel()) == 2 * got[1]            # every pair is in two rows of the table


@pytest.mark.parametrize("kind", ["balanced", "unequal5", "one", "null_cls", "singletons", "empty_classes", "many_declared"])
def test_classes(hip_ctx, kind):
    S, n = 130, 40
    X = _continuous(S, n)
    if kind == "balanced":
        cls, n_class = _balanced(S)
    elif kind == "unequal5":
        cls, n_class = _unequal5(S)
    elif kind in ("one", "null_cls"):
        cls, n_class = np.zeros(S, dtype=np.int32), 1
    elif kind == "singletons":
        cls, n_class = np.random.default_rng(1).permutation(S).astype(np.int32), S
    elif kind == "empty_classes":
        cls, n_class = (_unequal5(S)[0] * 3 + 1).astype(np.int32), 20     # labels 1, 4, 7, 10, 13 of 20
    else:   # more classes than a sample's bins have room for in LDS: the bins are added to in global memory (a 4 MB table)
        cls, n_class = (_unequal5(S)[0] * 500 + 7).astype(np.int32), 2049
        assert n_class > 2048
    if kind == "null_cls":
        ref = _reference(hip_ctx, ("cont", S, n), X, cls, 1, "one")
        got = hip_ctx.permdisp(X, None, 7)                              # n_class is ignored
        _assert_same(got, ref)
    else:
        got, ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, kind)
    assert got[2].shape == (S, n_class)
    if kind in ("one", "null_cls"):
        assert sum(int(v) for v in got[2][:, 0]) == 2 * got[1]
    if kind in ("empty_classes", "many_declared"):
        assert not np.delete(got[2], np.unique(cls), axis=1).any()      # empty classes stay 0 for every sample


@pytest.mark.parametrize("layout", ["sorted", "interleaved"])
def test_waves_of_one_class_and_of_two(hip_ctx, layout):
    """S = 300, two classes.  Class-sorted (0 x 150, 1 x 150): the waves of partners 0 .. 63, 64 .. 127, 192 .. 255 and
    256 .. 299 hold one class and take the wave's one atomic, the wave 128 .. 191 holds both; interleaved: every wave
    holds both.  The same matrix, so the two paths meet the same values."""
    S, n = 300, 40
    X = _continuous(S, n)
    cls = (np.arange(S) >= 150).astype(np.int32) if layout == "sorted" else (np.arange(S) % 2).astype(np.int32)
    _run(hip_ctx, ("cont", S, n), X, cls, 2, layout)


@pytest.mark.parametrize("spec", [None, "tkblock=1", "tkblock=1000"])
def test_block_cuts_give_identical_output(plan_ctx, spec):
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    plan_ctx.debug_set_plan(spec)
    _run(plan_ctx, ("cont", S, n), X, cls, n_class, "unequal5")


def test_heavy_ties(hip_ctx):
    """16 rows: a few hundred distinct taus among 32 896 pairs"""
    S = 257
    X = _few_rows(S, 16)
    cls, n_class = _unequal5(S)
    _run(hip_ctx, ("few", S), X, cls, n_class, "u5")


def test_na_pairs_add_nothing_and_the_table_is_as_summed(hip_ctx):
    """constant and all-missing columns: n_na > 0, the table holds the sums over the values"""
    X = _edge_matrix()
    cls = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3], dtype=np.int32)
    got, _ref = _run(hip_ctx, "edge", X, cls, 4, "four")
    assert got[0][1] > 0 and got[1] > 0 and got[2].any()
    assert not got[2][7].any()                                          # the all-missing column has no value at all


def test_no_value_at_all(hip_ctx):
    S, n = 20, 40
    X = np.asfortranarray(np.tile(np.arange(S, dtype=np.float64)[None, :], (n, 1)))   # every column constant
    cls, n_class = _balanced(S)
    got, _ref = _run(hip_ctx, "const", X, cls, n_class, "bal")
    assert got[0][0] == 0 and got[0][1] == S * (S - 1) // 2 and got[1] == 0 and not got[2].any()


def test_permanova_gives_the_same_totals_and_within_class_sums(hip_ctx):
    """an identity between two entries: no tolerance"""
    for key, X, cls, n_class in ((("cont", 130, 40), _continuous(130, 40), *_unequal5(130)),
                                 ("edge", _edge_matrix(), np.arange(12, dtype=np.int32) % 3, 3)):
        n_pairs, Q, T, mx, rc5 = hip_ctx.permdisp(X, cls, n_class)
        p_pairs, p_Q, p_class_q, p_mx, p_rc5 = hip_ctx.permanova(X, cls, n_class, None)
        assert np.array_equal(n_pairs, p_pairs) and Q == p_Q and mx == p_mx and np.array_equal(rc5, p_rc5)
        twice = [sum(int(T[i, c]) for i in np.flatnonzero(cls == c)) for c in range(n_class)]
        assert all(v % 2 == 0 for v in twice)
        if n_pairs[1] == 0:                                             # (with an NA pair PERMANOVA sums nothing)
            assert [v // 2 for v in twice] == list(p_class_q[0])
        else:
            assert not p_class_q.any()


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.permdisp(X64, *args)
    finally:
        ctx.f64_entries = False


def test_float32_row_major_view_matches_float64(hip_ctx):
    S, n = 65, 40
    rng = np.random.default_rng(21)
    X32 = np.ascontiguousarray(rng.standard_normal((n, S)).astype(np.float32))
    X32[rng.random((n, S)) < 0.08] = np.nan
    assert X32.flags.c_contiguous and _lib.input_view(X32)[2] == _lib.ORDER_ROW
    X64 = np.asfortranarray(X32, dtype=np.float64)
    cls, n_class = _unequal5(S)
    want = _f64_entry(hip_ctx, X64, cls, n_class)
    got = hip_ctx.permdisp(X32, cls, n_class)
    assert _same(got, want)
    _assert_same(got, _reference(hip_ctx, "f32", X64, cls, n_class, "u5"))


def test_scipy_csc_matches_dense(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    gna = [np.nan, np.inf, 0.0]
    cls, n_class = _unequal5(S)
    want = _f64_entry(hip_ctx, A.toarray(order="F"), cls, n_class, gna)
    got = hip_ctx.permdisp(A, cls, n_class, gna)
    assert _same(got, want)
    _assert_same(got, _reference(hip_ctx, "csc", X, cls, n_class, "u5", gna))


def test_a_used_context_equals_a_fresh_one(hip_ctx):
    """permanova, anosim and hclust leave other things in the kept plane, and a larger S and more classes leave larger
    buffers behind: the call directly after each of them equals the call on a context that has done nothing else"""
    S, n = 130, 40
    X = _continuous(S, n)
    big = _continuous(300, 40)
    cls, n_class = _unequal5(S)
    perms = documented_permutations(cls, 17, 7)
    fresh = _lib.Context(0)
    try:
        want = fresh.permdisp(X, cls, n_class)
    finally:
        fresh.close()
    _assert_same(want, _reference(hip_ctx, ("cont", S, n), X, cls, n_class, "unequal5"))
    cls_big = (np.arange(300) % 7).astype(np.int32)
    before = (lambda: hip_ctx.permanova(X, cls, n_class, perms),
              lambda: hip_ctx.anosim(X, cls, n_class, perms),
              lambda: hip_ctx.hclust(X, "average"),
              lambda: hip_ctx.permdisp(big, cls_big * 300, 2049),
              lambda: hip_ctx.permdisp(big, cls_big, 7))
    for other in before:
        other()
        assert _same(hip_ctx.permdisp(X, cls, n_class), want)


@pytest.mark.parametrize("kind", ["null", "side"])
def test_on_a_caller_stream(hip_ctx, kind):
    """the context on the caller's stream (icikt_ctx_set_stream), with the caller's own work queued in front"""
    import torch
    from tests.test_gpu_caller_stream import Lane
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    ref = _reference(hip_ctx, ("cont", S, n), X, cls, n_class, "unequal5")
    ctx = _lib.Context(0)
    try:
        lane = Lane(ctx, kind)
        with torch.cuda.stream(lane.ts):
            a = torch.ones(1 << 22, device="cuda")
            b = a + a                                                   # the caller's work, ahead of the call
        got = ctx.permdisp(X, cls, n_class)
        _assert_same(got, ref)
        with torch.cuda.stream(lane.ts):
            assert float(b[-1]) == 2.0
        assert _same(ctx.permdisp(X, cls, n_class), got)
    finally:
        ctx.close()


def test_refusals_leave_the_outputs_untouched(hip_ctx):
    S, n = 65, 40
    X = np.asfortranarray(_continuous(S, n))
    cls, n_class = _unequal5(S)
    L = _lib.lib()
    outs = {"n_pairs": np.full(2, -9, dtype=np.int64), "q_total": np.full(2, -9, dtype=np.int64),
            "t_lo": np.full(S * n_class, -9, dtype=np.int64), "t_hi": np.full(S * n_class, -9, dtype=np.int64)}

    def call(null=None, labels=cls, n_cls=n_class, perspective=1):
        ptr = {k: (None if k == null else _lib._ptr(a)) for k, a in outs.items()}
        rc = L.icikt_permdisp_f64(hip_ctx._h, _lib._ptr(X), n, S, n, None, 0, perspective, 0, 0, 0, _lib._ptr(labels), n_cls,
                                  ptr["n_pairs"], ptr["q_total"], ptr["t_lo"], ptr["t_hi"], None, None)
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == -1 and msg and msg.startswith(b"permdisp:"), (rc, msg)
        assert all(np.all(a == -9) for a in outs.values())
        return msg.decode()

    # 65 samples x 65 535 classes is within the cap; the cap needs more samples than a small test has, so it is met
    # with the shape alone: 1 100 columns of one row are refused before the matrix is read
    assert "n_class must be at least 1" in call(n_cls=0)
    assert "n_class exceeds 65535" in call(n_cls=65536)
    bad = cls.copy()
    bad[9] = n_class
    assert "cls[9] = 5 is outside 0 .. n_class - 1" in call(labels=bad)
    for name in outs:
        assert f"null output ({name})" in call(null=name)
    assert "perspective" in call(perspective=7)
    wide = np.zeros((1, 1100), order="F")
    lab = np.zeros(1100, dtype=np.int32)
    rc = L.icikt_permdisp_f64(hip_ctx._h, _lib._ptr(wide), 1, 1100, 1, None, 0, 1, 0, 0, 0, _lib._ptr(lab), 65535,
                              *(_lib._ptr(a) for a in outs.values()), None, None)
    assert rc == -1 and b"n_samp n_class exceeds ICIKT_PERMDISP_MAX_CELLS (67108864)" in L.icikt_last_error(hip_ctx._h)
    assert all(np.all(a == -9) for a in outs.values())
    with pytest.raises(_lib.IciktError, match="ICIKT_PERMDISP_MAX_CELLS"):
        hip_ctx.permdisp(wide, lab, 65535)
    _run(hip_ctx, ("cont", S, n), X, cls, n_class, "u5")                # the next call on the same context is right
    assert hip_ctx.num_pairs() == -1
    one = hip_ctx.permdisp(X[:, :1], np.zeros(1, dtype=np.int32), 1)
    assert list(one[0]) == [0, 0] and one[1] == 0 and one[2].tolist() == [[0]]


FLOATS = ("statistic", "pvalue", "ss_among", "ss_within", "perm_statistic", "distances", "class_mean_distance",
          "centroid_distance")


def _front_reference(ctx, key, X, codes, n_class, perms, lkey):
    full = _full(ctx, key, X)
    if (key, lkey, "front") not in _REF:
        _REF[(key, lkey, "front")] = brute_permdisp(full[0], codes, n_class, perms)
    return full, _REF[(key, lkey, "front")]


def _assert_front(got, full, ref):
    assert got["n_valid"] == ref["n_pairs"][0] and got["n_na"] == ref["n_pairs"][1]
    assert got["n_ge"] == ref["n_ge"] and got["n_undefined"] == ref["n_undefined"]
    assert (got["df_among"], got["df_within"]) == (ref["df_among"], ref["df_within"])
    assert got["sums"]["q_total"] == ref["q_total"] and got["sums"]["t"].tolist() == ref["t"]
    assert list(got["sums"]["class_q"]) == ref["class_q"]
    assert np.array_equal(got["class_size"], ref["class_size"])
    assert got["nearest_centroid"].dtype == np.int32 and np.array_equal(got["nearest_centroid"], ref["nearest_centroid"])
    assert got["n_negative"] == ref["n_negative"]
    for key in FLOATS:
        print(key, got[key] if np.ndim(got[key]) == 0 else np.ravel(got[key])[:4])
        assert np.shape(got[key]) == np.shape(ref[key]) and np.array_equal(bits(got[key]), bits(ref[key])), key
    assert got["max_taumax"] == full[1]


@pytest.mark.parametrize("strata", [None, "halves"])
def test_front_end_matches_the_checker(hip_ctx, strata):
    S, n = 65, 40
    X = _continuous(S, n)
    names = [f"s{i}" for i in range(S)]
    codes, _n = _unequal5(S)
    labels = [f"c{k}" for k in codes]                  # the levels sort as the codes do
    st = None if strata is None else ["l"] * 30 + ["r"] * 35
    got = api.ici_kendalltau_permdisp(X, labels, permutations=33, seed=11, strata=st, colnames=names)
    short = api.ici_kendalltau_permdisp(X, labels, permutations=33, seed=11, strata=st, colnames=names, return_perms=False)
    perms = documented_permutations(codes, 33, 11, st)
    full, ref = _front_reference(hip_ctx, ("cont", S, n), X, codes, 5, perms, ("front", strata))
    assert got["class_levels"] == [f"c{k}" for k in range(5)] and got["sample_id"] == names
    assert got["n_permutations"] == 33 and got["n_na"] == 0 and got["n_undefined"] == 0
    assert ref["exact"][0][0] is not None and (got["df_among"], got["df_within"]) == (4, 60)
    _assert_front(got, full, ref)
    assert "perm_statistic" not in short and bits(short["statistic"])[0] == bits(got["statistic"])[0]
    assert short["n_ge"] == got["n_ge"]
    # the same seed and strata: the labellings of the two other tests
    assert np.array_equal(api.anosim_permutations(codes, 33, 11, st), perms)
    again = api.ici_kendalltau_permdisp(X, labels, permutations=33, seed=11, strata=st, colnames=names)
    for key in FLOATS:
        assert np.array_equal(bits(again[key]), bits(got[key])), key


def test_front_end_with_na_pairs_warns_and_returns_na(hip_ctx):
    S, n = 65, 40
    X = _continuous(S, n).copy()
    X[:, 5] = np.nan                                   # an all-missing column: NA pairs
    names = [f"s{i}" for i in range(S)]
    codes, _n = _unequal5(S)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = api.ici_kendalltau_permdisp(X, [f"c{k}" for k in codes], permutations=17, seed=11, colnames=names)
    assert sum("PERMDISP needs every pair" in str(x.message) for x in w) == 1
    perms = documented_permutations(codes, 17, 11)
    full, ref = _front_reference(hip_ctx, "front-na", X, codes, 5, perms, "front-na")
    assert got["n_na"] == S - 1 and got["sums"]["t"].any() and not got["sums"]["t"][5].any()
    _assert_front(got, full, ref)
    for key in FLOATS:
        assert np.all(bits(got[key]) == bits(na_real())[0]), key
    assert np.all(got["nearest_centroid"] == -1) and got["n_ge"] == 0 and got["n_undefined"] == 17
