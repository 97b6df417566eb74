"""icikt_mantel_f64 / _in / _csc on the GPU: the Mantel test's integer sums of the identity and of every permutation.

The reference is the brute-force checker (tests/mantel_checker.py) applied to the raw plane of Context.matrix over all
pairs of the same data, computed once per data set.  Every integer must be EQUAL (n_valid, n_na, T of every labelling,
the four moments, n_ge, n_le, reason_counts), max_taumax equal, and every double of the front end BITWISE equal.  The
shapes are the smallest that reach each part: one pair, fewer pairs than a tile of the sort, several tiles, a strip of
the permutation kernel that ends one column before and 43 columns behind the 256-column boundary, and S = 1 100: past
the kernel's run of 1 024 rows and its fifth 256-column chunk.  The permutation counts are no multiple of the 16
permutations a workgroup takes.  At S = 300 the low limb of T is past 2^32 by itself: the carry between the limbs is in
every case."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.mantel_checker import bits, brute_mantel, documented_permutations
from tests.test_gpu_medians import _continuous
from tests.test_gpu_quantiles import _few_rows
from tests.test_gpu_topk import _edge_matrix

pytestmark = pytest.mark.gpu

METHODS = ["pearson", "spearman"]
_FULL = {}  # data key -> (raw [S, S], max_taumax, reason_counts) of Context.matrix: computed once
_REF = {}   # (data key, other key, method, permutations key) -> brute_mantel's dict


def _full(ctx, key, X, global_na=None):
    if key not in _FULL:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, "global", "two.sided", False, 0, True, True, want_keep=False)
        tm = out5[3][np.triu_indices(X.shape[1], k=1)]
        tm = tm[~np.isnan(tm)]
        _FULL[key] = (np.array(out5[1]), float(tm.max()) if tm.size else -np.inf, rc5)
    return _FULL[key]


def _reference(ctx, key, X, other, okey, method, perms, pkey, global_na=None):
    full = _full(ctx, key, X, global_na)
    rk = (key, okey, method, pkey)
    if rk not in _REF:
        _REF[rk] = brute_mantel(full[0], other, method, perms)
    return full, _REF[rk]


def _assert_same(got, ref):
    (_raw, mx_ref, rc_ref), r = ref
    n_pairs, T, mom, n_ge, n_le, mx, rc5 = got
    print("n_valid, n_na", list(n_pairs), list(r["n_pairs"]), "labellings", len(T), "differing T",
          sum(1 for a, b in zip(T, r["T"]) if a != b), "T[0]", T[0], r["T"][0], "moments", mom, r["moments"],
          "n_ge", n_ge, r["n_ge"], "n_le", n_le, r["n_le"])
    assert n_pairs.dtype == np.int64 and np.array_equal(n_pairs, r["n_pairs"])
    assert list(T) == r["T"] and tuple(mom) == r["moments"]
    assert n_ge == r["n_ge"] and n_le == r["n_le"]
    assert mx == mx_ref and np.array_equal(rc5, rc_ref)


def _other(S, kind, seed=3):
    """the condensed `other` of a data case"""
    P = S * (S - 1) // 2
    rng = np.random.default_rng(seed + S)
    if kind == "continuous":
        return rng.standard_normal(P) * 3.0 + 1.0                  # negative values among them
    if kind == "design":                                           # 0/1: two groups of samples
        g = rng.integers(0, 2, size=S)
        iu, ju = np.triu_indices(S, k=1)
        return (g[iu] != g[ju]).astype(np.float64)
    if kind == "levels5":
        return rng.integers(0, 5, size=P).astype(np.float64)
    if kind == "negative":
        return -np.abs(rng.standard_normal(P)) - 2.0
    if kind == "wide":                                             # 2^-20 .. 2^20
        v = np.ldexp(rng.uniform(0.5, 1.0, size=P), rng.integers(-19, 21, size=P))
        v[0], v[-1] = 2.0 ** -20, 2.0 ** 20
        return v
    if kind == "time":                                             # |t_i - t_j|
        t = rng.uniform(0.0, 100.0, size=S)
        iu, ju = np.triu_indices(S, k=1)
        return np.abs(t[iu] - t[ju])
    raise AssertionError(kind)


def _run(ctx, key, X, kind, method, n_perm, seed=7, global_na=None, **kw):
    S = X.shape[1]
    other = _other(S, kind)
    perms = documented_permutations(S, n_perm, seed)
    ref = _reference(ctx, key, X, other, kind, method, perms, (n_perm, seed), global_na)
    got = ctx.mantel(X, other, method, perms if n_perm else None, global_na, **kw)
    _assert_same(got, ref)
    return got, ref


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("S,n", [(2, 40), (3, 40), (65, 40), (130, 40), (257, 40), (300, 40), (130, 700), (1100, 40)])
def test_shapes(hip_ctx, S, n, method):
    X = _continuous(S, n)
    got, _ref = _run(hip_ctx, ("cont", S, n), X, "continuous", method, 5 if S == 1100 else 17)
    assert got[0][0] == S * (S - 1) // 2 and got[0][1] == 0
    if S >= 300:
        assert got[1][0] >= 1 << (64 if method == "pearson" else 40)     # far past what one 32-bit limb holds
    if S == 2:
        assert got[1][0] == got[1][1] and got[3] == got[4] == 17        # one pair: every permutation gives the same T


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n_perm", [0, 1, 5, 17, 33])
def test_permutation_counts(hip_ctx, n_perm, method):
    S, n = 65, 40
    X = _continuous(S, n)
    got, _ref = _run(hip_ctx, ("cont", S, n), X, "time", method, n_perm)
    assert got[1].shape == (1 + n_perm,)
    if n_perm == 0:
        assert got[3] == 0 and got[4] == 0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("spec", [None, "tkblock=1", "padjtile=4", "padjtile=100", "anostrip=1", "anostrip=64", "anostrip=300",
                                  "anoperms=3", "tkblock=1,padjtile=100,anostrip=64,anoperms=3"])
def test_plans_give_identical_output(plan_ctx, spec, method):
    """the block cut, the sort's tile, the strip and the batch change nothing: every plan gives the checker's integers"""
    S, n = 130, 40
    X = _continuous(S, n)
    plan_ctx.debug_set_plan(spec)
    _run(plan_ctx, ("cont", S, n), X, "levels5", method, 33)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("spec", ["anostrip=1", "anostrip=64", "anostrip=300", None])
def test_strips_past_one_chunk(plan_ctx, spec, method):
    """S = 300: with the default strip a second strip of 44 columns, with a strip of 300 a second 256-column chunk"""
    S, n = 300, 40
    X = _continuous(S, n)
    plan_ctx.debug_set_plan(spec)
    _run(plan_ctx, ("cont", S, n), X, "continuous", method, 5)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["design", "levels5", "negative", "wide"])
def test_other_cases(hip_ctx, kind, method):
    S, n = 130, 40
    X = _continuous(S, n)
    got, ref = _run(hip_ctx, ("cont", S, n), X, kind, method, 33)
    if kind == "design" and method == "pearson":
        assert set(ref[1]["yv"].tolist()) == {0, 2 ** 30}
    if kind == "wide" and method == "pearson":
        assert ref[1]["yv"].min() == 0 and ref[1]["yv"].max() > 2 ** 30


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("spec", [None, "padjtile=64,tkblock=1"])
def test_heavy_ties_in_both(plan_ctx, spec, method):
    """16 rows: a few hundred distinct taus among 32 896 pairs, against a 0/1 design: runs of equal keys across the
    sort's tiles in x and two values in y, and equal T among the permutations' sums"""
    S = 257
    X = _few_rows(S, 16)
    plan_ctx.debug_set_plan(spec)
    got, ref = _run(plan_ctx, ("few", S), X, "design", method, 5)
    assert len(np.unique(ref[1]["xv"])) < 2000 and len(np.unique(ref[1]["yv"])) == 2


@pytest.mark.parametrize("method", METHODS)
def test_equal_sums_under_a_design_matrix(hip_ctx, method):
    """permutations that only move samples inside their group reproduce T exactly: they count in n_ge AND in n_le"""
    S, n = 65, 40
    X = _continuous(S, n)
    other = _other(S, "design")
    g = np.random.default_rng(3 + S).integers(0, 2, size=S)
    strata = [int(v) for v in g]
    perms = documented_permutations(S, 17, 5, strata)                  # within the groups
    perms = np.vstack([perms, documented_permutations(S, 16, 6)])      # and free ones
    ref = _reference(hip_ctx, ("cont", S, n), X, other, "design", method, perms, "within+free")
    got = hip_ctx.mantel(X, other, method, perms)
    _assert_same(got, ref)
    assert all(t == got[1][0] for t in got[1][1:18]) and got[3] >= 17 and got[4] >= 17 and got[3] + got[4] >= 33 + 17


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("spec", [None, "anostrip=1,anoperms=3"])
def test_na_pairs_sum_nothing(plan_ctx, spec, method):
    """constant and all-missing columns: n_na > 0, every T and moment is 0; the permutations are still checked"""
    X = _edge_matrix()
    plan_ctx.debug_set_plan(spec)
    got, _ref = _run(plan_ctx, "edge", X, "continuous", method, 33)
    assert got[0][1] > 0 and not any(got[1]) and got[2] == (0, 0, 0, 0) and got[3] == got[4] == 0
    bad = documented_permutations(X.shape[1], 33, 7)
    bad[20, 3] = bad[20, 4]
    with pytest.raises(_lib.IciktError, match=r"mantel: perms\[20\]\[4\] = \d+ occurs twice"):
        plan_ctx.mantel(X, _other(X.shape[1], "continuous"), method, bad)


@pytest.mark.parametrize("method", METHODS)
def test_no_value_at_all(hip_ctx, method):
    S, n = 20, 40
    X = np.asfortranarray(np.tile(np.arange(S, dtype=np.float64)[None, :], (n, 1)))   # every column constant
    got, _ref = _run(hip_ctx, "const", X, "continuous", method, 5)
    assert got[0][0] == 0 and got[0][1] == S * (S - 1) // 2 and not any(got[1]) and got[3] == got[4] == 0


@pytest.mark.parametrize("method", METHODS)
def test_all_values_equal_and_constant_other(hip_ctx, method):
    """identical columns: every raw is the same double (no digit to sort by); then a constant other: r is undefined"""
    S, n = 66, 40
    col = np.random.default_rng(3).standard_normal(n)
    X = np.asfortranarray(np.tile(col[:, None], (1, S)))
    got, ref = _run(hip_ctx, "same", X, "continuous", method, 5)
    assert len(set(ref[1]["xv"].tolist())) == 1 and got[3] == got[4] == 5
    assert api.mantel_statistic(S * (S - 1) // 2, got[1][0], *got[2]) is None
    X2 = _continuous(65, 40)
    const = np.full(65 * 64 // 2, -4.5)
    perms = documented_permutations(65, 5, 7)
    got2 = hip_ctx.mantel(X2, const, method, perms)
    _assert_same(got2, _reference(hip_ctx, ("cont", 65, 40), X2, const, "const", method, perms, (5, 7)))
    assert got2[3] == got2[4] == 5 and api.mantel_statistic(65 * 64 // 2, got2[1][0], *got2[2]) is None


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.mantel(X64, *args)
    finally:
        ctx.f64_entries = False


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and list(a[1]) == list(b[1]) and a[2] == b[2] and a[3:6] == b[3:6]
            and np.array_equal(a[6], b[6]))


@pytest.mark.parametrize("method", METHODS)
def test_float32_row_major_view_matches_float64(hip_ctx, method):
    S, n = 65, 40
    rng = np.random.default_rng(21)
    X32 = np.ascontiguousarray(rng.standard_normal((n, S)).astype(np.float32))
    X32[rng.random((n, S)) < 0.08] = np.nan
    assert X32.flags.c_contiguous and _lib.input_view(X32)[2] == _lib.ORDER_ROW
    X64 = np.asfortranarray(X32, dtype=np.float64)
    other, perms = _other(S, "time"), documented_permutations(S, 17, 7)
    want = _f64_entry(hip_ctx, X64, other, method, perms)
    got = hip_ctx.mantel(X32, other, method, perms)
    assert _same(got, want)
    _assert_same(got, _reference(hip_ctx, "f32", X64, other, "time", method, perms, (17, 7)))


@pytest.mark.parametrize("method", METHODS)
def test_scipy_csc_matches_dense(hip_ctx, method):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    gna = [np.nan, np.inf, 0.0]
    other, perms = _other(S, "time"), documented_permutations(S, 17, 7)
    want = _f64_entry(hip_ctx, A.toarray(order="F"), other, method, perms, gna)
    got = hip_ctx.mantel(A, other, method, perms, gna)
    assert _same(got, want)
    _assert_same(got, _reference(hip_ctx, "csc", X, other, "time", method, perms, (17, 7), gna))


def test_refusals_leave_the_outputs_and_the_context(hip_ctx):
    S, n = 65, 40
    P = S * (S - 1) // 2
    X = _continuous(S, n)
    other, perms = _other(S, "time"), documented_permutations(S, 17, 7)
    twice = perms.copy()
    twice[9, 40] = twice[9, 12]
    with pytest.raises(_lib.IciktError, match=rf"mantel: perms\[9\]\[40\] = {twice[9, 12]} occurs twice"):
        hip_ctx.mantel(X, other, "pearson", twice)
    outside = perms.copy()
    outside[-1, -1] = S
    with pytest.raises(_lib.IciktError, match=r"mantel: perms\[16\]\[64\] = 65 is outside 0 \.\. S - 1 \(S = 65\)"):
        hip_ctx.mantel(X, other, "spearman", outside)
    outside[-1, -1] = -1
    with pytest.raises(_lib.IciktError, match=r"mantel: perms\[16\]\[64\] = -1 is outside 0 \.\. S - 1"):
        hip_ctx.mantel(X, other, "pearson", outside)
    hole = other.copy()
    hole[1234] = np.nan
    with pytest.raises(_lib.IciktError, match=r"mantel: other\[1234\] is not finite"):
        hip_ctx.mantel(X, hole, "spearman", perms)
    hole[1234] = -np.inf
    with pytest.raises(_lib.IciktError, match=r"mantel: other\[1234\] is not finite"):
        hip_ctx.mantel(X, hole, "pearson", perms)
    wide = other.copy()
    wide[0], wide[1] = -1.5e308, 1.5e308
    with pytest.raises(_lib.IciktError, match="mantel: the span of other is not finite"):
        hip_ctx.mantel(X, wide, "pearson", perms)
    with pytest.raises(_lib.IciktError, match="mantel: method must be"):
        hip_ctx.mantel(X, other, 2, perms)
    with pytest.raises(_lib.IciktError, match="mantel: perspective"):
        hip_ctx.mantel(X, other, "pearson", perms, perspective="sideways")

    L = _lib.lib()
    Xf = np.asfortranarray(X)
    outs = {"n_pairs": np.full(2, -9, dtype=np.int64), "t_lo": np.full(18, -9, dtype=np.int64),
            "t_hi": np.full(18, -9, dtype=np.int64), "moments": np.full(8, -9, dtype=np.int64),
            "n_ge": np.full(1, -9, dtype=np.int64), "n_le": np.full(1, -9, dtype=np.int64)}
    mx, rc5 = np.full(1, -9.0), np.full(5, -9, dtype=np.int64)

    def call(n_perm=17, null=None, perm_a=perms, other_a=other, method=0):
        ptr = {k: (None if k == null else _lib._ptr(a)) for k, a in outs.items()}
        rc = L.icikt_mantel_f64(hip_ctx._h, _lib._ptr(Xf), n, S, n, None, 0, 1, 0, 0, 0, _lib._ptr(other_a), method,
                                _lib._ptr(perm_a), n_perm, ptr["n_pairs"], ptr["t_lo"], ptr["t_hi"], ptr["moments"],
                                ptr["n_ge"], ptr["n_le"], _lib._ptr(mx), _lib._ptr(rc5))
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == -1 and msg and msg.startswith(b"mantel:"), (rc, msg)
        assert all(np.all(a == -9) for a in outs.values()) and mx[0] == -9.0 and np.all(rc5 == -9)
        return msg.decode()

    assert "n_perm must not be negative" in call(-1)
    assert "ICIKT_MANTEL_MAX_PERM" in call(1000001)
    assert "null perms" in call(perm_a=None)
    assert "null other" in call(other_a=None)
    assert "occurs twice" in call(perm_a=twice)
    assert "is outside 0 .. S - 1" in call(perm_a=outside)
    assert "other[1234] is not finite" in call(other_a=hole)
    assert "method must be" in call(method=7)
    for name in outs:
        assert f"null output ({name})" in call(null=name)
    # the next valid call is the checker's
    _run(hip_ctx, ("cont", S, n), X, "time", "pearson", 17)
    _run(hip_ctx, ("cont", S, n), X, "time", "spearman", 17)
    assert hip_ctx.num_pairs() == -1
    rc = L.icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
    assert rc == -5, rc                                # ICIKT_E_STATE: the call leaves nothing prepared
    one = hip_ctx.mantel(X[:, :1], np.zeros(0), "pearson", np.zeros((3, 1), dtype=np.int32))
    assert list(one[0]) == [0, 0] and list(one[1]) == [0, 0, 0, 0] and one[2] == (0, 0, 0, 0)
    assert P == other.shape[0]


@pytest.mark.parametrize("method", METHODS)
def test_context_reuse_matches_a_fresh_context(method):
    """mantel directly after anosim, permanova, padjust and pcoa, and after a larger and a smaller matrix, on one
    context: what the entries before left in the shared planes and in the table does not show"""
    S, n = 130, 40
    X = _continuous(S, n)
    other, perms = _other(S, "time"), documented_permutations(S, 17, 7)
    cls = (np.arange(S) % 3).astype(np.int32)
    labs = api.anosim_permutations(cls, 5, seed=1)
    fresh = _lib.Context(0)
    try:
        want = fresh.mantel(X, other, method, perms)
    finally:
        fresh.close()
    ctx = _lib.Context(0)
    try:
        for before in (lambda: ctx.anosim(X, cls, 3, labs), lambda: ctx.permanova(X, cls, 3, labs),
                       lambda: ctx.padjust(X, "BH", [0.05]), lambda: ctx.pcoa(X, k=3),
                       lambda: ctx.mantel(_continuous(257, 40), _other(257, "levels5"), method, documented_permutations(257, 3, 2)),
                       lambda: ctx.mantel(_continuous(65, 40), _other(65, "design"), method, documented_permutations(65, 3, 2)),
                       lambda: ctx.mantel(X, _other(S, "wide"), "spearman" if method == "pearson" else "pearson", perms)):
            before()
            assert _same(ctx.mantel(X, other, method, perms), want)
    finally:
        ctx.close()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("strata", [None, "halves"])
def test_front_end_matches_the_checker(hip_ctx, strata, method):
    S, n = 65, 40
    X = _continuous(S, n)
    names = [f"s{i}" for i in range(S)]
    t = np.random.default_rng(12).uniform(0, 50, size=S)
    other = np.abs(t[:, None] - t[None, :])
    st = None if strata is None else ["l"] * 30 + ["r"] * 35
    got = api.ici_kendalltau_mantel(X, other, method=method, permutations=33, seed=11, strata=st, colnames=names)
    short = api.ici_kendalltau_mantel(X, other, method=method, permutations=33, seed=11, strata=st, colnames=names,
                                      return_perms=False)
    perms = documented_permutations(S, 33, 11, st)
    full, ref = _reference(hip_ctx, ("cont", S, n), X, other, "front", method, perms, ("front", strata))
    assert got["sample_id"] == names and got["method"] == method and got["n_permutations"] == 33
    assert got["n_valid"] == ref["n_pairs"][0] == S * (S - 1) // 2 and got["n_na"] == 0
    assert got["n_ge"] == ref["n_ge"] and got["n_le"] == ref["n_le"]
    assert list(got["sums"]["T"]) == ref["T"]
    assert (got["sums"]["sx"], got["sums"]["sxx"], got["sums"]["sy"], got["sums"]["syy"]) == ref["moments"]
    for key in ("statistic", "pvalue", "perm_statistic"):
        print(key, got[key] if np.ndim(got[key]) == 0 else got[key][:4])
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
    assert got["max_taumax"] == full[1]
    assert "perm_statistic" not in short and bits(short["statistic"])[0] == bits(got["statistic"])[0]
    assert short["n_ge"] == got["n_ge"]


def test_front_end_na_pairs(hip_ctx):
    S, n = 65, 40
    X = _continuous(S, n).copy()
    X[:, 5] = 1.5                                      # a constant column: NA pairs, the warnings
    names = [f"s{i}" for i in range(S)]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = api.ici_kendalltau_mantel(X, _other(S, "time"), permutations=5, seed=1, colnames=names)
    assert any("`ici_kendalltau_medians` returns `n_valid`" in str(x.message) for x in w)
    na = bits(api._na_real())[0]
    assert got["n_na"] == S - 1 and got["n_valid"] == S * (S - 1) // 2 - (S - 1) and got["n_ge"] == got["n_le"] == 0
    assert bits(got["statistic"])[0] == na and bits(got["pvalue"])[0] == na and np.all(bits(got["perm_statistic"]) == na)
