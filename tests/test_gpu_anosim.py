"""icikt_anosim_f64 / _in / _csc on the GPU: ANOSIM's rank sums of the observed labelling and of every permutation.

The reference is the brute-force checker (tests/anosim_checker.py: sort + searchsorted ranks, masked sums, Python-int
fractions) applied to the raw plane of Context.matrix over all pairs, computed once per data set.  Every integer must
be EQUAL (M, n_na, W2 and nW of every labelling, n_ge, n_undefined, the per-class sums, reason_counts), max_taumax
equal, and every double of the front end BITWISE equal.  The shapes are the smallest that reach each part: one pair,
fewer pairs than a tile of the sort, several tiles, a strip of the permutation kernel that ends one column before and
43 columns behind the 256-column boundary, more than one run of rows; the permutation counts are no multiple of the 16
labellings a workgroup takes."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.anosim_checker import bits, brute_anosim, documented_permutations
from tests.test_gpu_medians import _continuous
from tests.test_gpu_quantiles import _few_rows
from tests.test_gpu_topk import _edge_matrix

pytestmark = pytest.mark.gpu

_FULL = {}  # data key -> (raw [S, S], max_taumax, reason_counts) of Context.matrix: computed once
_REF = {}   # (data key, labels key) -> brute_anosim's dict


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
        _REF[(key, lkey)] = brute_anosim(full[0], cls, n_class, perms)
    return full, _REF[(key, lkey)]


def _assert_same(got, ref):
    (_raw, mx_ref, rc_ref), r = ref
    n_pairs, w2, nw, n_ge, n_undef, class_w2, class_nw, mx, rc5 = got
    print("M, n_na", list(n_pairs), list(r["n_pairs"]), "labellings", len(w2), "differing w2", int(np.sum(w2 != r["w2"])),
          "differing nw", int(np.sum(nw != r["nw"])), "n_ge", n_ge, r["n_ge"], "n_undefined", n_undef, r["n_undefined"])
    for a in (n_pairs, w2, nw, class_w2, class_nw):
        assert a.dtype == np.int64
    assert np.array_equal(n_pairs, r["n_pairs"])
    assert np.array_equal(w2, r["w2"]) and np.array_equal(nw, r["nw"])
    assert n_ge == r["n_ge"] and n_undef == r["n_undefined"]
    assert np.array_equal(class_w2, r["class_w2"]) and np.array_equal(class_nw, r["class_nw"])
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


def _run(ctx, key, X, cls, n_class, n_perm, lkey, seed=7, global_na=None, **kw):
    perms = documented_permutations(cls, n_perm, seed)
    ref = _reference(ctx, key, X, cls, n_class, perms, (lkey, n_perm, seed), global_na)
    got = ctx.anosim(X, cls, n_class, perms if n_perm else None, global_na, **kw)
    _assert_same(got, ref)
    return got, ref


@pytest.mark.parametrize("S,n", [(2, 40), (3, 40), (65, 40), (130, 40), (257, 40), (300, 40), (130, 700)])
def test_shapes(hip_ctx, S, n):
    X = _continuous(S, n)
    cls, n_class = _balanced(S)
    got, _ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, 17, "bal")
    assert got[0][0] == S * (S - 1) // 2 and got[0][1] == 0
    if S == 2:
        assert got[2][0] == 0 and got[4] == 17           # the one pair lies between the classes: no labelling has an R


@pytest.mark.parametrize("kind", ["balanced", "unequal5", "one", "singletons", "empty_classes"])
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
    else:
        cls, n_class = (_unequal5(S)[0] * 3 + 1).astype(np.int32), 20     # labels 1, 4, 7, 10, 13 of 20
    got, ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, 17, kind)
    if kind == "one":
        assert got[2][0] == S * (S - 1) // 2 and got[3] == 0 and got[4] == 17
    if kind == "singletons":
        assert got[2][0] == 0 and got[3] == 0 and got[4] == 17 and not got[5].any()
    if kind == "empty_classes":
        assert got[5].shape == (20,) and np.count_nonzero(got[6]) == 4    # (the singleton has no within pair)
    if kind in ("balanced", "unequal5"):
        assert ref[1]["exact"][0] is not None and got[4] == 0


@pytest.mark.parametrize("n_perm", [0, 1, 5, 17, 33])
def test_permutation_counts(hip_ctx, n_perm):
    S, n = 65, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    got, _ref = _run(hip_ctx, ("cont", S, n), X, cls, n_class, n_perm, "u5")
    assert got[1].shape == (1 + n_perm,)
    if n_perm == 0:
        assert got[3] == 0 and got[4] == 0


def test_999_permutations(hip_ctx):
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    _run(hip_ctx, ("cont", S, n), X, cls, n_class, 999, "u5")


@pytest.mark.parametrize("spec", [None, "tkblock=1", "padjtile=4", "padjtile=64", "padjtile=100", "anostrip=1",
                                  "anostrip=64", "anoperms=1", "anoperms=3", "tkblock=1,padjtile=100,anostrip=64,anoperms=3"])
def test_plans_give_identical_output(plan_ctx, spec):
    """the block cut, the sort's tile, the strip and the batch change nothing: every plan gives the checker's integers"""
    S, n = 130, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    plan_ctx.debug_set_plan(spec)
    _run(plan_ctx, ("cont", S, n), X, cls, n_class, 33, "u5")


@pytest.mark.parametrize("spec", ["anostrip=1", "anostrip=64", "anostrip=300", None])
def test_strips_past_one_row_run(plan_ctx, spec):
    """S = 300: two runs of 256 rows, and with the default strip a second strip of 44 columns"""
    S, n = 300, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    plan_ctx.debug_set_plan(spec)
    _run(plan_ctx, ("cont", S, n), X, cls, n_class, 5, "u5")


def test_plan_key_ranges(plan_ctx):
    for spec, word in (("anostrip=0", "anostrip"), ("anostrip=4097", "anostrip"), ("anoperms=0", "anoperms"),
                       ("anoperms=1048577", "anoperms")):
        with pytest.raises(_lib.IciktError, match=word + " must be in 1"):
            plan_ctx.debug_set_plan(spec)
    plan_ctx.debug_set_plan("anostrip=4096,anoperms=1048576")


@pytest.mark.parametrize("spec", [None, "padjtile=64,tkblock=1"])
def test_heavy_ties(plan_ctx, spec):
    """16 rows: a few hundred distinct taus among 32 896 pairs, runs of equal keys across the sort's tiles"""
    S = 257
    X = _few_rows(S, 16)
    cls, n_class = _unequal5(S)
    plan_ctx.debug_set_plan(spec)
    got, ref = _run(plan_ctx, ("few", S), X, cls, n_class, 5, "u5")
    assert len(np.unique(ref[1]["r2"])) < 2000


@pytest.mark.parametrize("spec", [None, "anostrip=1,anoperms=3"])
def test_na_pairs_count_nw_on_the_device(plan_ctx, spec):
    """constant and all-missing columns: n_na > 0, so nW is counted by the kernel; with classes of the NA columns'
    partners some labellings differ in nW"""
    X = _edge_matrix()
    S = X.shape[1]
    cls = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3], dtype=np.int32)
    plan_ctx.debug_set_plan(spec)
    got, ref = _run(plan_ctx, "edge", X, cls, 4, 33, "four")
    assert got[0][1] > 0 and len(set(got[2].tolist())) > 1


def test_no_value_at_all(hip_ctx):
    S, n = 20, 40
    X = np.asfortranarray(np.tile(np.arange(S, dtype=np.float64)[None, :], (n, 1)))   # every column constant
    cls, n_class = _balanced(S)
    got, _ref = _run(hip_ctx, "const", X, cls, n_class, 5, "bal")
    assert got[0][0] == 0 and got[0][1] == S * (S - 1) // 2
    assert not got[1].any() and not got[2].any() and got[3] == 0 and got[4] == 5


def test_all_values_equal(hip_ctx):
    """identical columns: every raw is the same double, no digit to sort by, every doubled rank is M + 1, R = 0"""
    S, n = 66, 40
    col = np.random.default_rng(3).standard_normal(n)
    X = np.asfortranarray(np.tile(col[:, None], (1, S)))
    cls, n_class = _unequal5(S)
    got, ref = _run(hip_ctx, "same", X, cls, n_class, 5, "u5")
    M = S * (S - 1) // 2
    assert set(ref[1]["r2"].tolist()) == {M + 1} and ref[1]["exact"][0] == 0 and got[3] == 5


def test_planted_classes_separate(hip_ctx):
    S, n = 64, 60
    rng = np.random.default_rng(8)
    cls, n_class = _balanced(S)
    factor = rng.standard_normal((n, 2))
    X = np.asfortranarray(2.0 * factor[:, cls] + rng.standard_normal((n, S)))
    got, ref = _run(hip_ctx, "planted", X, cls, n_class, 33, "bal")
    assert ref[1]["statistic"] > 0.5 and ref[1]["n_ge"] == 0 and ref[1]["pvalue"] == 1 / 34
    assert got[3] == 0


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.anosim(X64, *args)
    finally:
        ctx.f64_entries = False


def _same(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in (0, 1, 2, 5, 6, 8)) and a[3] == b[3] and a[4] == b[4] and a[7] == b[7])


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
    got = hip_ctx.anosim(X32, cls, n_class, perms)
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
    got = hip_ctx.anosim(A, cls, n_class, perms, gna)
    assert _same(got, want)
    _assert_same(got, _reference(hip_ctx, "csc", X, cls, n_class, perms, "u5", gna))


def test_argument_errors_leave_the_context_usable(hip_ctx):
    S, n = 65, 40
    X = _continuous(S, n)
    cls, n_class = _unequal5(S)
    perms = documented_permutations(cls, 17, 7)
    bad = cls.copy()
    bad[9] = n_class
    with pytest.raises(_lib.IciktError, match=r"anosim: cls\[9\] = 5 is outside 0 \.\. n_class - 1"):
        hip_ctx.anosim(X, bad, n_class, perms)
    badp = perms.copy()
    badp[-1, -1] = -1
    with pytest.raises(_lib.IciktError, match=r"anosim: perm_cls\[16\]\[64\] = -1 is outside 0 \.\. n_class - 1"):
        hip_ctx.anosim(X, cls, n_class, badp)
    with pytest.raises(_lib.IciktError, match="anosim: perspective"):
        hip_ctx.anosim(X, cls, n_class, perms, perspective="sideways")

    L = _lib.lib()
    Xf = np.asfortranarray(X)
    outs = {"n_pairs": np.full(2, -9, dtype=np.int64), "w2": np.full(18, -9, dtype=np.int64),
            "nw": np.full(18, -9, dtype=np.int64), "n_ge": np.full(1, -9, dtype=np.int64),
            "n_undefined": np.full(1, -9, dtype=np.int64), "class_w2": np.full(n_class, -9, dtype=np.int64),
            "class_nw": np.full(n_class, -9, dtype=np.int64)}

    def call(n_perm, null=None, perm_ptr=_lib._ptr(perms)):
        ptr = {k: (None if k == null else _lib._ptr(a)) for k, a in outs.items()}
        rc = L.icikt_anosim_f64(hip_ctx._h, _lib._ptr(Xf), n, S, n, None, 0, 1, 0, 0, 0, _lib._ptr(cls), n_class, perm_ptr,
                                n_perm, ptr["n_pairs"], ptr["w2"], ptr["nw"], ptr["n_ge"], ptr["n_undefined"],
                                ptr["class_w2"], ptr["class_nw"], None, None)
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == -1 and msg and msg.startswith(b"anosim:"), (rc, msg)
        assert all(np.all(a == -9) for a in outs.values())
        return msg.decode()

    assert "n_perm must not be negative" in call(-1)
    assert "ICIKT_ANOSIM_MAX_PERM" in call(1000001)
    assert "null perm_cls" in call(17, perm_ptr=None)
    for name in outs:
        assert f"null output ({name})" in call(17, null=name)
    # the next valid call is the checker's
    _run(hip_ctx, ("cont", S, n), X, cls, n_class, 17, "u5")
    assert hip_ctx.num_pairs() == -1
    rc = L.icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
    assert rc == -5, rc                                # ICIKT_E_STATE: the call leaves nothing prepared
    one = hip_ctx.anosim(X[:, :1], np.zeros(1, dtype=np.int32), 1, np.zeros((3, 1), dtype=np.int32))
    assert list(one[0]) == [0, 0] and not one[1].any() and one[3] == 0 and one[4] == 3


@pytest.mark.parametrize("strata", [None, "halves"])
def test_front_end_matches_the_checker(hip_ctx, strata):
    S, n = 65, 40
    X = _continuous(S, n)
    X[:, 5] = 1.5                                      # a constant column: NA pairs, the warning
    names = [f"s{i}" for i in range(S)]
    codes, _n = _unequal5(S)
    labels = [f"c{k}" for k in codes]                  # the levels sort as the codes do
    st = None if strata is None else ["l"] * 30 + ["r"] * 35
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = api.ici_kendalltau_anosim(X, labels, permutations=33, seed=11, strata=st, colnames=names)
        short = api.ici_kendalltau_anosim(X, labels, permutations=33, seed=11, strata=st, colnames=names, return_perms=False)
    assert any(str(x.message) in _lib.REASON_WARNINGS.values() for x in w)
    perms = documented_permutations(codes, 33, 11, st)
    full, ref = _reference(hip_ctx, "front", X, codes, 5, perms, ("front", strata))
    assert got["class_levels"] == [f"c{k}" for k in range(5)] and got["sample_id"] == names
    assert got["n_permutations"] == 33 and got["n_valid"] == ref["n_pairs"][0] and got["n_na"] == ref["n_pairs"][1] == S - 1
    assert got["n_ge"] == ref["n_ge"] and got["n_undefined"] == ref["n_undefined"]
    for key in ("w2", "nw", "class_w2", "class_nw"):
        assert np.array_equal(got["sums"][key], ref[key]), key
    for key in ("statistic", "pvalue", "perm_statistic", "class_mean_rank", "within_mean_rank", "between_mean_rank"):
        print(key, got[key] if np.ndim(got[key]) == 0 else got[key][:4])
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
    assert got["max_taumax"] == full[1]
    assert "perm_statistic" not in short and bits(short["statistic"])[0] == bits(got["statistic"])[0]
    assert short["n_ge"] == got["n_ge"]
