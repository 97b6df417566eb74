"""icikt_permanova_f64 / _in / _csc on the GPU: PERMANOVA's fixed-point sums per class of the observed labelling and of
every permutation.

The reference is the brute-force checker (tests/permanova_checker.py: plain loops, Python ints and Fractions) applied to
the raw plane of Context.matrix over all pairs, computed once per data set and labelling.  Every integer must be EQUAL
(the values and NA pairs, Q, A_c of every labelling and class with the limbs combined, reason_counts), max_taumax equal,
and every double of the front end BITWISE equal.  The shapes are the smallest that reach each part: one pair, a strip
of the permutation kernel that ends one column before and 43 columns behind the 256-column boundary, more than one run
of its 1 024 rows (S = 1 100), class bins in LDS and in global memory; the permutation counts are no multiple of the 16 labellings a
workgroup takes."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.permanova_checker import bits, brute_permanova, documented_permutations, na_real
from tests.test_gpu_medians import _continuous
from tests.test_gpu_quantiles import _few_rows
from tests.test_gpu_topk import _edge_matrix

pytestmark = pytest.mark.gpu

_FULL = {}  # data key -> (raw [S, S], max_taumax, reason_counts) of Context.matrix: computed once
_REF = {}   # (data key, labels key) -> brute_permanova's dict


def _full(ctx, key, X, global_na=None):
    if key not in _FULL:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, "global", "two.sided", False, 0, True, True, want_keep=False)
        tm = out5[3][np.triu_indices(X.shape[1], k=1)]
        tm = tm[~np.isnan(tm)]
        _FULL[key] = (np.array(out5[1]), float(tm.max()) if tm.size else -np.inf, rc5)
    return _FULL[key]


def _reference(ctx, key, X, cls, n_class, perms, lkey, global_na=None):
    full = _full(ctx, key, X, global_na)
    if (key, lkey) not in _REF:
        _REF[(key, lkey)] = brute_permanova(full[0], cls, n_class, perms)
    return full, _REF[(key, lkey)]


def _assert_same(got, ref):
    (_raw, mx_ref, rc_ref), r = ref
    n_pairs, Q, class_q, mx, rc5 = got
    want = np.array(r["class_q"], dtype=object).reshape(class_q.shape)
    print("values, n_na", list(n_pairs), list(r["n_pairs"]), "Q", Q, r["q_total"], "cells", class_q.size,
          "differing cells", int(np.sum(class_q != want)))
    assert n_pairs.dtype == np.int64 and np.array_equal(n_pairs, r["n_pairs"])
    assert isinstance(Q, int) and Q == r["q_total"]
    assert class_q.dtype == object and all(isinstance(v, int) for v in class_q.ravel())
    assert class_q.tolist() == r["class_q"]
    assert mx == mx_ref and np.array_equal(rc5, rc_ref)


def _balanced(S):
    return (np.arange(S) % 2).astype(np.int32), 2


def _unequal5(S):
    """five classes of unequal size in shuffled order, class 3 a singleton"""
    cls = np.zeros(S, dtype=np.int32)
    cls[S // 3:] = 1
    cls[S // 2:] = 2
    cls[-1] = 3
    cls[S - 1 - S // 5:S - 1] = 4
    np.random.default_rng(4).shuffle(cls)
    assert np.sum(cls == 3) == 1 and len(np.unique(cls)) == 5
    return cls, 5


def _run(ctx, key, X, cls, n_class, n_perm, lkey, seed=7, global_na=None, strata=None, **kw):
    perms = documented_permutations(cls, n_perm, seed, strata)
    ref = _reference(ctx, key, X, cls, n_class, perms, (lkey, n_perm, seed), global_na)
    got = ctx.permanova(X, cls, n_class, perms if n_perm else None, global_na, **kw)
    _assert_same(got, ref)
    return got, ref


@pytest.mark.parametrize("S,n", [(2, 40), (3, 40), (65, 40), (130, 40), (257, 40), (300, 40), (130, 700)])
def test_shapes(hip_ctx, S, n):
    X = _continuous(S, n)
    cls, n_class = _balanced(S)
    got, ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, 17, "bal")
    assert got[0][0] == S * (S - 1) // 2 and got[0][1] == 0
    assert got[2].shape == (18, 2)
    if S == 2:
        assert not got[2].any() and ref[1]["n_undefined"] == 17      # the one pair lies between the classes; S = C'
    else:
        assert got[2][0][0] > 0 and ref[1]["exact"][0][0] is not None      # (S = 3: class 1 is a singleton)
        assert S == 3 or got[2][0].all()


@pytest.mark.parametrize("kind", ["balanced", "unequal5", "one", "singletons", "empty_classes", "many_declared"])
def test_classes(hip_ctx, kind):
    S, n = 130, 40
    X = _continuous(S, n)
    if kind == "balanced":
        cls, n_class = _balanced(S)
    elif kind == "unequal5":
        cls, n_class = _unequal5(S)
    elif kind == "one":
        cls, n_class = np.zeros(S, dtype=np.int32), 1
    elif kind == "singletons":
        cls, n_class = np.random.default_rng(1).permutation(S).astype(np.int32), S
    elif kind == "empty_classes":
        cls, n_class = (_unequal5(S)[0] * 3 + 1).astype(np.int32), 20     # labels 1, 4, 7, 10, 13 of 20
    else:   # more classes than a labelling's bins have room for in LDS: the bins are added to in global memory
        cls, n_class = (_unequal5(S)[0] * 600 + 7).astype(np.int32), 2500
        assert n_class > 2048
    got, ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, 17, kind)
    Q = got[1]
    if kind == "one":
        assert all(row[0] == Q for row in got[2]) and ref[1]["n_undefined"] == 17
    if kind == "singletons":
        assert not got[2].any() and ref[1]["n_undefined"] == 17
    if kind in ("empty_classes", "many_declared"):
        used = np.unique(cls)
        assert got[2].shape == (18, n_class)
        assert np.count_nonzero(got[2][0]) == 4                           # (the singleton has no within pair)
        assert not np.delete(got[2], used, axis=1).any()                  # empty bins stay 0 in every labelling
    if kind in ("balanced", "unequal5"):
        assert ref[1]["exact"][0][0] is not None and ref[1]["n_undefined"] == 0


@pytest.mark.parametrize("n_perm", [0, 1, 5, 17, 33])
def test_permutation_counts(hip_ctx, n_perm):
    S, n = 65, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    got, _ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, n_perm, "u5")
    assert got[2].shape == (1 + n_perm, 5)


@pytest.mark.parametrize("spec", [None, "anoperms=16", "anoperms=3", "anostrip=1", "anostrip=64", "anostrip=213",
                                  "tkblock=1", "tkblock=1000", "tkblock=1,anostrip=64,anoperms=16"])
def test_plans_give_identical_output(plan_ctx, spec):
    """the block cut, the strip and the batch change nothing: every plan gives the checker's integers"""
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    plan_ctx.debug_set_plan(spec)
    _run(plan_ctx, ("cont", S, n), X, cls, n_class, 33, "u5")


@pytest.mark.parametrize("spec", ["anostrip=1", "anostrip=64", "anostrip=213", None])
def test_strips_past_256_columns(plan_ctx, spec):
    """S = 300: with the default strip a second strip of 44 columns; strips of 1, 64 and 213 columns beside it"""
    S, n = 300, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    plan_ctx.debug_set_plan(spec)
    _run(plan_ctx, ("cont", S, n), X, cls, n_class, 5, "u5")


def test_more_than_one_run_of_rows(hip_ctx):
    """the permutation kernel's run is 1 024 rows: S = 1 100 is the smallest round shape whose columns past 1 025 are
    summed by two workgroups each, which meet in the column sums.  Two labellings keep the checker's loops short."""
    S, n = 1100, 24
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    got, _ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, 1, "u5")
    assert got[0][1] == 0 and np.count_nonzero(got[2]) == 8          # (summed on the device; the singleton's bins stay 0)


def test_heavy_ties(hip_ctx):
    """16 rows: a few hundred distinct taus among 32 896 pairs"""
    S = 257
    X = _few_rows(S, 16)
    cls, n_class = _unequal5(S)
    _run(hip_ctx, ("few", S), X, cls, n_class, 5, "u5")


def test_strata(hip_ctx):
    S, n = 65, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    st = ["l"] * 30 + ["r"] * 35
    got, ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, 17, "u5-strata", strata=st)
    perms = documented_permutations(cls, 17, 7, st)
    for row in perms:   # permuted within the strata: the class sizes of each stratum are the observed ones
        assert np.array_equal(np.bincount(row[:30], minlength=5), np.bincount(cls[:30], minlength=5))


def test_supplied_labellings_with_other_class_sizes(hip_ctx):
    S, n = 65, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    rng = np.random.default_rng(31)
    perms = np.vstack([rng.integers(0, n_class, size=(18, S)), (cls[None, :] + 1) % n_class, cls[None, :]]).astype(np.int32)
    ref = _reference(hip_ctx, ("cont", S, n), X, cls, n_class, perms, "supplied")
    got = hip_ctx.permanova(X, cls, n_class, perms)
    _assert_same(got, ref)
    names = [f"s{i}" for i in range(S)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = api.ici_kendalltau_permanova(X, [f"c{k}" for k in cls], permutations=perms, colnames=names)
    r = ref[1]
    assert any(s != r["sizes"][0] for s in r["sizes"][1:19])              # compared through the F fraction
    assert res["n_ge"] == r["n_ge"] >= 2 and res["n_undefined"] == r["n_undefined"]   # the renamed and the observed one count
    for key in ("statistic", "pvalue", "perm_statistic"):
        assert np.array_equal(bits(res[key]), bits(r[key])), key


@pytest.mark.parametrize("spec", [None, "anostrip=1,anoperms=3"])
def test_na_pairs_give_zero_bins(plan_ctx, spec):
    """constant and all-missing columns: n_na > 0, nothing is summed per class, the labels are still checked"""
    X = _edge_matrix()
    S = X.shape[1]
    cls = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3], dtype=np.int32)
    plan_ctx.debug_set_plan(spec)
    got, ref = _run(plan_ctx, "edge", X, cls, 4, 33, "four")
    assert got[0][1] > 0 and got[1] > 0 and not got[2].any() and got[2].shape == (34, 4)
    perms = documented_permutations(cls, 33, 7)
    perms[20, 3] = 4
    with pytest.raises(_lib.IciktError, match=r"permanova: perm_cls\[20\]\[3\] = 4 is outside 0 \.\. n_class - 1"):
        plan_ctx.permanova(X, cls, 4, perms)


def test_no_value_at_all(hip_ctx):
    S, n = 20, 40
    X = np.asfortranarray(np.tile(np.arange(S, dtype=np.float64)[None, :], (n, 1)))   # every column constant
    cls, n_class = _balanced(S)
    got, _ref = _run(hip_ctx, "const", X, cls, n_class, 5, "bal")
    assert got[0][0] == 0 and got[0][1] == S * (S - 1) // 2 and got[1] == 0 and not got[2].any()


def test_identical_columns_have_no_dissimilarity(hip_ctx):
    S, n = 66, 40
    col = np.random.default_rng(3).standard_normal(n)
    X = np.asfortranarray(np.tile(col[:, None], (1, S)))
    cls, n_class = _unequal5(S)
    got, ref = _run(hip_ctx, "same", X, cls, n_class, 5, "u5")
    assert got[1] == 0 and not got[2].any() and ref[1]["exact"][0][0] is None     # raw = 1 everywhere: SS_T = 0


def test_bad_label_in_the_second_batch(plan_ctx):
    S, n = 65, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    perms = documented_permutations(cls, 33, 7)
    bad = cls.copy()
    bad[9] = n_class
    with pytest.raises(_lib.IciktError, match=r"permanova: cls\[9\] = 5 is outside 0 \.\. n_class - 1"):
        plan_ctx.permanova(X, bad, n_class, perms)
    plan_ctx.debug_set_plan("anoperms=16")
    badp = perms.copy()
    badp[20, 64] = -1                      # labelling 21 of 34: the second batch of 16, behind a batch that has run
    with pytest.raises(_lib.IciktError, match=r"permanova: perm_cls\[20\]\[64\] = -1 is outside 0 \.\. n_class - 1 \(n_class = 5\)"):
        plan_ctx.permanova(X, cls, n_class, badp)
    with pytest.raises(_lib.IciktError, match="permanova: perspective"):
        plan_ctx.permanova(X, cls, n_class, perms, perspective="sideways")
    _run(plan_ctx, ("cont", S, n), X, cls, n_class, 33, "u5")          # the next call on the same context is right
    assert plan_ctx.num_pairs() == -1


def test_refusals_leave_the_outputs_untouched(hip_ctx):
    S, n = 65, 40
    X = np.asfortranarray(_continuous(S, n))
    cls, n_class = _unequal5(S)
    perms = documented_permutations(cls, 17, 7)
    L = _lib.lib()
    outs = {"n_pairs": np.full(2, -9, dtype=np.int64), "q_total": np.full(2, -9, dtype=np.int64),
            "bins_lo": np.full(18 * n_class, -9, dtype=np.int64), "bins_hi": np.full(18 * n_class, -9, dtype=np.int64)}

    def call(n_perm, null=None, perm_ptr=_lib._ptr(perms), n_cls=n_class):
        ptr = {k: (None if k == null else _lib._ptr(a)) for k, a in outs.items()}
        rc = L.icikt_permanova_f64(hip_ctx._h, _lib._ptr(X), n, S, n, None, 0, 1, 0, 0, 0, _lib._ptr(cls), n_cls, perm_ptr,
                                   n_perm, ptr["n_pairs"], ptr["q_total"], ptr["bins_lo"], ptr["bins_hi"], None, None)
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == -1 and msg and msg.startswith(b"permanova:"), (rc, msg)
        assert all(np.all(a == -9) for a in outs.values())
        return msg.decode()

    assert "n_perm must not be negative" in call(-1)
    assert "ICIKT_ANOSIM_MAX_PERM" in call(1000001)
    assert "ICIKT_PERMANOVA_MAX_CELLS" in call(999999, n_cls=65535)
    assert "n_class exceeds 65535" in call(17, n_cls=65536)
    assert "null perm_cls" in call(17, perm_ptr=None)
    for name in outs:
        assert f"null output ({name})" in call(17, null=name)
    badp = perms.copy()
    badp[-1, -1] = 7
    assert "perm_cls[16][64] = 7" in call(17, perm_ptr=_lib._ptr(badp))
    _run(hip_ctx, ("cont", S, n), X, cls, n_class, 17, "u5")
    one = hip_ctx.permanova(X[:, :1], np.zeros(1, dtype=np.int32), 1, np.zeros((3, 1), dtype=np.int32))
    assert list(one[0]) == [0, 0] and one[1] == 0 and one[2].shape == (4, 1) and not one[2].any()


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.permanova(X64, *args)
    finally:
        ctx.f64_entries = False


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2].tolist() == b[2].tolist() and a[3] == b[3]
            and np.array_equal(a[4], b[4]))


def test_float32_row_major_view_matches_float64(hip_ctx):
    S, n = 65, 40
    rng = np.random.default_rng(21)
    X32 = np.ascontiguousarray(rng.standard_normal((n, S)).astype(np.float32))
    X32[rng.random((n, S)) < 0.08] = np.nan
    assert X32.flags.c_contiguous and _lib.input_view(X32)[2] == _lib.ORDER_ROW
    X64 = np.asfortranarray(X32, dtype=np.float64)
    cls, n_class = _unequal5(S)
    perms = documented_permutations(cls, 17, 7)
    want = _f64_entry(hip_ctx, X64, cls, n_class, perms)
    got = hip_ctx.permanova(X32, cls, n_class, perms)
    assert _same(got, want)
    _assert_same(got, _reference(hip_ctx, "f32", X64, cls, n_class, perms, "u5"))


def test_scipy_csc_matches_dense(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    gna = [np.nan, np.inf, 0.0]
    cls, n_class = _unequal5(S)
    perms = documented_permutations(cls, 17, 7)
    want = _f64_entry(hip_ctx, A.toarray(order="F"), cls, n_class, perms, gna)
    got = hip_ctx.permanova(A, cls, n_class, perms, gna)
    assert _same(got, want)
    _assert_same(got, _reference(hip_ctx, "csc", X, cls, n_class, perms, "u5", gna))


def test_a_used_context_equals_a_fresh_one(hip_ctx):
    """anosim, padjust and hclust leave other things in the kept plane and in plane_a, and a larger S leaves larger
    buffers behind: the call directly after each of them equals the call on a context that has done nothing else"""
    S, n = 130, 40
    X = _continuous(S, n)
    big = _continuous(300, 40)
    cls, n_class = _unequal5(S)
    perms = documented_permutations(cls, 17, 7)
    fresh = _lib.Context(0)
    try:
        want = fresh.permanova(X, cls, n_class, perms)
    finally:
        fresh.close()
    _assert_same(want, _reference(hip_ctx, ("cont", S, n), X, cls, n_class, perms, ("u5", 17, 7)))
    cls_big, _c = _unequal5(300)
    before = (lambda: hip_ctx.anosim(X, cls, n_class, perms),
              lambda: hip_ctx.padjust(X, "BH", [0.05]),
              lambda: hip_ctx.hclust(X, "average"),
              lambda: hip_ctx.permanova(big, cls_big, 5, documented_permutations(cls_big, 5, 7)))
    for other in before:
        other()
        assert _same(hip_ctx.permanova(X, cls, n_class, perms), want)


def test_the_same_call_twice_gives_identical_bits(hip_ctx):
    S, n = 130, 40
    X = _continuous(S, n)
    names = [f"s{i}" for i in range(S)]
    labels = [f"c{k}" for k in _unequal5(S)[0]]
    a = api.ici_kendalltau_permanova(X, labels, permutations=33, seed=11, colnames=names)
    b = api.ici_kendalltau_permanova(X, labels, permutations=33, seed=11, colnames=names)
    assert list(a) == list(b)
    for key in ("statistic", "r2", "pvalue", "ss_total", "ss_within", "ss_among", "perm_statistic", "class_ss"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    assert a["sums"]["q_total"] == b["sums"]["q_total"] and a["sums"]["class_q"].tolist() == b["sums"]["class_q"].tolist()


@pytest.mark.parametrize("strata", [None, "halves"])
def test_front_end_matches_the_checker(hip_ctx, strata):
    S, n = 65, 40
    X = _continuous(S, n)
    names = [f"s{i}" for i in range(S)]
    codes, _n = _unequal5(S)
    labels = [f"c{k}" for k in codes]                  # the levels sort as the codes do
    st = None if strata is None else ["l"] * 30 + ["r"] * 35
    got = api.ici_kendalltau_permanova(X, labels, permutations=33, seed=11, strata=st, colnames=names)
    short = api.ici_kendalltau_permanova(X, labels, permutations=33, seed=11, strata=st, colnames=names, return_perms=False)
    perms = documented_permutations(codes, 33, 11, st)
    full, ref = _reference(hip_ctx, ("cont", S, n), X, codes, 5, perms, ("front", strata))
    assert got["class_levels"] == [f"c{k}" for k in range(5)] and got["sample_id"] == names
    assert got["n_permutations"] == 33 and got["n_valid"] == ref["n_pairs"][0] and got["n_na"] == 0
    assert got["n_ge"] == ref["n_ge"] and got["n_undefined"] == ref["n_undefined"] == 0
    assert (got["df_among"], got["df_within"]) == (ref["df_among"], ref["df_within"]) == (4, 60)
    assert got["sums"]["q_total"] == ref["q_total"] and got["sums"]["class_q"].tolist() == ref["class_q"]
    assert np.array_equal(got["class_size"], ref["class_size"])
    for key in ("statistic", "r2", "pvalue", "ss_total", "ss_within", "ss_among", "perm_statistic", "class_ss"):
        print(key, got[key] if np.ndim(got[key]) == 0 else got[key][:4])
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
    assert got["max_taumax"] == full[1]
    assert "perm_statistic" not in short and bits(short["statistic"])[0] == bits(got["statistic"])[0]
    assert short["n_ge"] == got["n_ge"]
    # the same seed and strata: ANOSIM's labellings
    assert np.array_equal(api.anosim_permutations(codes, 33, 11, st), perms)


def test_front_end_with_na_pairs_warns_and_returns_na(hip_ctx):
    S, n = 65, 40
    X = _continuous(S, n).copy()
    X[:, 5] = 1.5                                      # a constant column: NA pairs
    names = [f"s{i}" for i in range(S)]
    codes, _n = _unequal5(S)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = api.ici_kendalltau_permanova(X, [f"c{k}" for k in codes], permutations=17, seed=11, colnames=names)
    assert sum("PERMANOVA needs every pair" in str(x.message) for x in w) == 1
    assert any(str(x.message) in _lib.REASON_WARNINGS.values() for x in w)
    perms = documented_permutations(codes, 17, 11)
    _full_, ref = _reference(hip_ctx, "front-na", X, codes, 5, perms, "front-na")
    assert got["n_na"] == ref["n_pairs"][1] == S - 1 and got["n_valid"] == ref["n_pairs"][0]
    assert got["sums"]["q_total"] == ref["q_total"] and not got["sums"]["class_q"].any()
    assert got["n_ge"] == 0 and got["n_undefined"] == 17
    for key in ("statistic", "r2", "pvalue", "ss_total", "ss_within", "ss_among", "perm_statistic", "class_ss"):
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
        assert np.all(bits(got[key]) == bits(na_real())[0]), key
