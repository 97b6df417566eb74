"""icikt_padjust_f64 / _in / _csc on the GPU: R's p.adjust over the p-values of all pairs, sorted, scanned and cut on the
device.

The reference is the brute-force checker (tests/padjust_checker.py) applied to Context.matrix on the same input: every
double -- cut-offs, table -- must be BITWISE equal (a cut-off without a rejection carries R's NA_real_ bits), every count
equal.  The shapes are the smallest that reach each part of the kernels: one pair, fewer keys than a tile, several
tiles, tiles that end one key before, at and after the plane's end, enough tiles for several rounds of the scans' top
level, runs of equal keys across tile borders, NA keys, no test at all, every key equal (no digit to sort by)."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.padjust_checker import ALPHAS, METHODS, NA_REAL_BITS, bits, brute_padjust
from tests.test_gpu_medians import _continuous
from tests.test_gpu_quantiles import _few_rows
from tests.test_gpu_topk import _edge_matrix

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float64).tiny
_OUT5 = {}   # (data key, perspective, alternative, continuity) -> (out5, max_taumax, reason_counts): computed once
_REF = {}    # (..., method) -> the checker's answer


def _matrices(ctx, key, X, global_na=None, perspective="global", alternative="two.sided", continuity=False):
    mk = (key, perspective, alternative, continuity)
    if mk not in _OUT5:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, perspective, alternative, continuity, 0, True, True,
                                      want_keep=False)
        iu, ju = np.triu_indices(X.shape[1], k=1)
        tm = out5[3][iu, ju]
        tm = tm[~np.isnan(tm)]
        _OUT5[mk] = (out5, float(tm.max()) if tm.size else -np.inf, rc5)
    return _OUT5[mk]


def _correlated(S, n, seed=12):
    """one shared factor with loadings in [0, 0.9): at S = 130, n = 40 BH rejects 13 / 152 / 2 389 of the 8 385 pairs
    at 0.01 / 0.05 / 0.5 and the other methods 6 / 9 / 29 (the CPU oracle's figures)"""
    rng = np.random.default_rng(seed + 1000 * S + n)
    f = rng.standard_normal(n)
    load = rng.uniform(0.0, 0.9, S)
    X = np.asfortranarray(f[:, None] * load[None, :] + rng.standard_normal((n, S)) * np.sqrt(1.0 - load ** 2)[None, :])
    X[rng.random((n, S)) < 0.08] = np.nan
    return X


def _reference(ctx, key, X, method, alphas=ALPHAS, **kw):
    out5, mx, rc5 = _matrices(ctx, key, X, **kw)
    rk = (key, kw.get("perspective", "global"), kw.get("alternative", "two.sided"), kw.get("continuity", False), method,
          tuple(alphas))
    if rk not in _REF:
        ref = brute_padjust(out5[2], method, alphas)
        ref["max_taumax"], ref["reason_counts"] = mx, rc5
        _REF[rk] = ref
    return _REF[rk]


def _assert_same(got, ref):
    n_tests, n_rej, cutoff, table, n_table, mx, rc5 = got
    print("n_tests", n_tests, "n_rejected", n_rej, ref["n_rejected"], "n_table", n_table, ref["n_table"],
          "differing cells", int(np.sum(bits(cutoff) != bits(ref["p_cutoff"]))),
          int(np.sum(bits(table[0]) != bits(ref["table_p"]))) if table.shape[1] == ref["n_table"] else "shape",
          int(np.sum(bits(table[1]) != bits(ref["table_adjusted"]))) if table.shape[1] == ref["n_table"] else "shape")
    assert np.array_equal(n_tests, ref["n_tests"])
    assert np.array_equal(n_rej, ref["n_rejected"])
    assert np.array_equal(bits(cutoff), bits(ref["p_cutoff"]))
    assert np.array_equal(bits(cutoff) == NA_REAL_BITS, n_rej == 0)
    assert n_table == ref["n_table"] and table.shape == (2, n_table)
    assert np.array_equal(bits(table[0]), bits(ref["table_p"]))
    assert np.array_equal(bits(table[1]), bits(ref["table_adjusted"]))
    assert mx == ref["max_taumax"]
    assert np.array_equal(rc5, ref["reason_counts"])


def _same_bits(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray) and x.dtype == np.float64:
            assert np.array_equal(bits(x), bits(y))
        else:
            assert np.array_equal(x, y)


def _run(ctx, X, method, alphas=ALPHAS, **kw):
    S = X.shape[1]
    return ctx.padjust(X, method, alphas, max(S * (S - 1) // 2, 1), **kw)


@pytest.mark.parametrize("n", [40, 700])
@pytest.mark.parametrize("S", [2, 3, 65, 130])
def test_small_and_mid_shapes(hip_ctx, S, n):
    """1, 3, 2 080 and 8 385 pairs at the library's tile: one key, fewer keys than a tile, several tiles"""
    X = _continuous(S, n)
    for method in METHODS:
        ref = _reference(hip_ctx, ("cont", S, n), X, method)
        got = _run(hip_ctx, X, method)
        _assert_same(got, ref)
        assert got[0][0] == S * (S - 1) // 2 and got[1][-1] == got[0][0]      # alpha = 1 rejects every test
        assert got[4] == len(np.unique(ref["sorted_p"]))


def test_tiles_and_block_cuts_give_identical_output(plan_ctx):
    """S = 130, P = 8 385: tiles of 4 keys (2 097 tiles, 525 chunks of counters: three rounds of the offset scan's
    top level), of 64 and of 100 keys, tiles that end one key before, at and after the plane's end, and a row per block
    against one block"""
    S, n = 130, 40
    P = S * (S - 1) // 2
    # (random columns reject nothing below alpha = 1; the correlated ones, without that alpha, give a table and cut-offs
    #  that end inside the plane: at 2 389 of 8 385 sorted positions for BH)
    for method, key, alphas in [(m, "cont", ALPHAS) for m in METHODS] + [(m, "corr", (0.01, 0.05, 0.5)) for m in METHODS]:
        X = _continuous(S, n) if key == "cont" else _correlated(S, n)
        ref = _reference(plan_ctx, (key, S, n), X, method, alphas)
        if key == "corr":
            assert 0 < ref["n_rejected"][0] < ref["n_rejected"][1] < ref["n_rejected"][2] < P
        outs = []
        for spec in (None, "padjtile=4", "padjtile=64", "padjtile=100", f"padjtile={P - 1}", f"padjtile={P}",
                     f"padjtile={P + 1}", "tkblock=1", "tkblock=1,padjtile=33", "tkblock=1000,padjtile=4"):
            if method != "BH" and spec not in (None, "padjtile=4", "tkblock=1,padjtile=33"):
                continue                                   # (the sort does not know the method: the full list once)
            plan_ctx.debug_set_plan(spec)
            outs.append(_run(plan_ctx, X, method, alphas))
            _assert_same(outs[-1], ref)
        for got in outs[1:]:
            _same_bits(got, outs[0])
    with pytest.raises(_lib.IciktError, match="padjtile"):
        plan_ctx.debug_set_plan("padjtile=0")


@pytest.mark.parametrize("spec", [None, "padjtile=50"])
def test_equal_values(plan_ctx, spec):
    """16 rows give a few hundred distinct p-values among 1.1 million pairs: runs of equal keys thousands long across
    tile borders, a table much shorter than n_rejected, and (tiles of 50 keys) 22 rounds of the offset scan's top level
    and 5 of the min / max scan's"""
    S = 1500
    X = _few_rows(S)
    plan_ctx.debug_set_plan(spec)
    for method in METHODS:
        ref = _reference(plan_ctx, ("few", S, 16), X, method)
        assert ref["n_table"] < 1000 and ref["n_rejected"].max() > 100 * ref["n_table"]
        _assert_same(_run(plan_ctx, X, method), ref)


@pytest.mark.parametrize("cfg", [("global", "two.sided", False), ("local", "less", True)])
def test_na_pairs(plan_ctx, cfg):
    """the constant and the all-missing column are NA with every partner: NA keys are sorted last and are no tests"""
    perspective, alternative, continuity = cfg
    kw = {"perspective": perspective, "alternative": alternative, "continuity": continuity}
    X = _edge_matrix()
    S = X.shape[1]
    for method in METHODS:
        ref = _reference(plan_ctx, "edge", X, method, **kw)
        assert ref["n_tests"][1] >= 2 * (S - 2) + 1 and ref["n_tests"][0] > 0
        for spec in (None, "tkblock=3,padjtile=7"):
            plan_ctx.debug_set_plan(spec)
            _assert_same(_run(plan_ctx, X, method, **kw), ref)


def test_no_test_at_all(hip_ctx):
    """every column constant: every pair has a reason code, m = 0"""
    S, n = 9, 30
    X = np.asfortranarray(np.tile(np.arange(1.0, S + 1.0), (n, 1)))
    for method in METHODS:
        ref = _reference(hip_ctx, "const", X, method)
        assert ref["n_tests"].tolist() == [0, S * (S - 1) // 2]
        got = _run(hip_ctx, X, method)
        _assert_same(got, ref)
        assert not got[1].any() and np.all(bits(got[2]) == NA_REAL_BITS) and got[4] == 0


def test_two_rows(hip_ctx):
    """2-row input: pairs without a reason code whose p-value is NaN are dropped as p.adjust drops an NA"""
    rng = np.random.default_rng(33)
    X = np.asfortranarray(rng.standard_normal((2, 9)))
    out5, _mx, rc5 = _matrices(hip_ctx, "tworow", X)
    tri = out5[2][np.triu_indices(9, k=1)]
    print("reason counts", rc5, "NaN p-values", int(np.isnan(tri).sum()))
    assert rc5[0] > 0 and int(np.isnan(tri).sum()) > int(rc5[1:].sum())      # a NaN p with reason code 0
    for method in METHODS:
        _assert_same(_run(hip_ctx, X, method), _reference(hip_ctx, "tworow", X, method))


def _tail_matrix(n=660):
    """a sorted column, its copy, copies with the first k = 40 .. 100 values reversed (tau falls by k (k - 1) / C(n, 2):
    p runs from exactly 0 up to 1e-290), and eight random columns.  The CPU oracle puts the last zero at k = 72 and
    1.4e-306 at k = 76."""
    rng = np.random.default_rng(7)
    a = np.sort(rng.standard_normal(n))
    cols = [a, a.copy()]
    for k in range(40, 101, 2):
        c = a.copy()
        c[:k] = c[:k][::-1]
        cols.append(c)
    for _ in range(8):
        cols.append(rng.standard_normal(n))
    return np.asfortranarray(np.column_stack(cols))


def test_zero_and_subnormal_p_values(plan_ctx):
    """A run of zeros leads the order (Holm's running maximum starts from 0, the table stores +0), and the smallest
    p-values the library gives follow.  No p-value of the library is subnormal: its pnorm is R's, which returns 0 beyond
    |z| = 37.5193, and 2 pnorm(-37.5193) = 5.4e-308 is above the smallest normal double 2.2e-308 (measured on the
    device: 420 of these 820 pairs are 0, the smallest positive p is 5.36e-308).  Subnormal values reach the formulas
    in tests/test_padjust_host.py only."""
    X = _tail_matrix()
    S = X.shape[1]
    out5, _mx, _rc5 = _matrices(plan_ctx, "tail", X)
    tri = out5[2][np.triu_indices(S, k=1)]
    n_zero, n_sub = int(np.sum(tri == 0.0)), int(np.sum((tri > 0.0) & (tri < TINY)))
    print("pairs", tri.size, "p == 0:", n_zero, "subnormal p:", n_sub, "smallest positive p:", tri[tri > 0].min())
    assert n_zero > 1 and int(np.sum((tri > 0.0) & (tri < 1e-300))) > 1
    for method in METHODS:
        ref = _reference(plan_ctx, "tail", X, method)
        for spec in (None, "padjtile=16"):
            plan_ctx.debug_set_plan(spec)
            got = _run(plan_ctx, X, method)
            _assert_same(got, ref)
            assert bits(got[3][0])[0] == 0 and bits(got[3][1])[0] == 0       # +0, adjusted to +0
            assert got[1][0] == n_zero and bits(got[2])[0] == 0              # alpha = 0 rejects the zeros


def test_every_p_equal(hip_ctx):
    """identical columns: one run of equal keys, and every digit the same in all keys -- no pass of the sort runs"""
    S, n = 12, 40
    a = np.random.default_rng(34).standard_normal(n)
    X = np.asfortranarray(np.tile(a[:, None], (1, S)))
    for method in METHODS:
        ref = _reference(hip_ctx, "equal", X, method)
        assert ref["n_table"] == 1 and ref["n_tests"][1] == 0
        _assert_same(_run(hip_ctx, X, method), ref)


def _raw_call(ctx, X, method, alphas, max_table, table, null=None, n_alpha=None, perspective=1):
    """icikt_padjust_f64 itself, on the caller's arrays"""
    L = _lib.lib()
    n_feat, n_samp = X.shape
    alphas = np.ascontiguousarray(alphas, dtype=np.float64)
    outs = {"n_tests": np.full(2, -7, dtype=np.int64), "n_rejected": np.full(20, -7, dtype=np.int64),
            "p_cutoff": np.full(20, 123.25), "n_table": np.full(1, -7, dtype=np.int64)}
    mx = np.full(1, 55.5)
    rc5 = np.full(5, -9, dtype=np.int64)
    ptr = {k: (None if k == null else _lib._ptr(v)) for k, v in outs.items()}
    rc = L.icikt_padjust_f64(ctx._h, _lib._ptr(X), n_feat, n_samp, max(n_feat, 1), None, 0, perspective, 0, 0, 0, method,
                             None if null == "alpha" else _lib._ptr(alphas),
                             len(alphas) if n_alpha is None else n_alpha, max_table,
                             ptr["n_tests"], ptr["n_rejected"], ptr["p_cutoff"],
                             None if (table is None or null == "table") else _lib._ptr(table), ptr["n_table"],
                             _lib._ptr(mx), _lib._ptr(rc5))
    return rc, outs, mx, rc5


def test_table_capacity(hip_ctx):
    """max_table = 0, 1, n_table - 1, n_table, n_table + 5: the first min(n_table, max_table) entries of each plane are
    written, every slot behind them keeps the caller's bytes"""
    S, n = 65, 40
    X = _continuous(S, n)
    ref = _reference(hip_ctx, ("cont", S, n), X, "BH")
    nt = ref["n_table"]
    assert nt > 5
    for room in (0, 1, nt - 1, nt, nt + 5):
        table = np.full((2, room), 123.25) if room else None
        rc, outs, _mx, _rc5 = _raw_call(hip_ctx, X, _lib.ADJUST["BH"], ALPHAS, room, table)
        assert rc == 0 and outs["n_table"][0] == nt
        assert np.array_equal(outs["n_rejected"][:len(ALPHAS)], ref["n_rejected"]) and np.all(outs["n_rejected"][len(ALPHAS):] == -7)
        assert np.array_equal(bits(outs["p_cutoff"][:len(ALPHAS)]), bits(ref["p_cutoff"])) and np.all(outs["p_cutoff"][len(ALPHAS):] == 123.25)
        k = min(room, nt)
        if room:
            assert np.array_equal(bits(table[0, :k]), bits(ref["table_p"][:k]))
            assert np.array_equal(bits(table[1, :k]), bits(ref["table_adjusted"][:k]))
            assert np.all(table[:, k:] == 123.25)
    got = hip_ctx.padjust(X, "BH", ALPHAS, 3)
    assert got[4] == nt and got[3].shape == (2, 3) and np.array_equal(bits(got[3][0]), bits(ref["table_p"][:3]))
    assert hip_ctx.padjust(X, "BH", ALPHAS)[3].shape == (2, 0)


def _f64_entry(ctx, X64, *args):
    ctx.f64_entries = True
    try:
        return ctx.padjust(X64, *args)
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
        want = _f64_entry(hip_ctx, X64, method, ALPHAS, 4000)
        got = hip_ctx.padjust(X32, method, ALPHAS, 4000)
        _same_bits(got, want)
        _assert_same(got, _reference(hip_ctx, "f32", X64, method))


def test_scipy_csc_matches_dense(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    A = sp.csc_matrix(X)
    gna = [np.nan, np.inf, 0.0]
    for method in METHODS:
        want = _f64_entry(hip_ctx, X, method, ALPHAS, 4000, gna)
        got = hip_ctx.padjust(A, method, ALPHAS, 4000, gna)
        _same_bits(got, want)
        _assert_same(got, _reference(hip_ctx, "csc", X, method, global_na=gna))


@pytest.mark.parametrize("method", ["BH", "holm"])
def test_significant_front_end(hip_ctx, method):
    """the edge set is the brute-force `adjusted <= alpha` selection in combn order, the adjusted column the checker's"""
    S, n = 130, 40
    X = _correlated(S, n)
    names = [f"s{i}" for i in range(S)]
    alpha = 0.05
    out5, _mx, _rc5 = _matrices(hip_ctx, ("corr", S, n), X, global_na=None)
    ref = brute_padjust(out5[2], method, (alpha,))
    iu, ju = np.triu_indices(S, k=1)
    tri = out5[2][iu, ju] + 0.0
    tri_adj = ref["adjusted"][np.searchsorted(ref["sorted_p"], tri)]        # (no NaN p in this matrix)
    assert np.array_equal(bits(ref["sorted_p"][np.searchsorted(ref["sorted_p"], tri)]), bits(tri))
    keep = tri_adj <= alpha
    assert 0 < keep.sum() < tri.size
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = api.ici_kendalltau_significant(X, alpha=alpha, method=method, global_na=(np.nan,), colnames=names,
                                             engine=api.HipEngine())
        adj = api.ici_kendalltau_padjust(X, method=method, alpha=(alpha, 1.0), global_na=(np.nan,), colnames=names,
                                         engine=api.HipEngine())
    print("rejected", int(keep.sum()), "of", tri.size, "edges", res["n_edges"])
    assert np.array_equal(res["i"], iu[keep]) and np.array_equal(res["j"], ju[keep])
    assert np.array_equal(bits(res["adjusted"]), bits(tri_adj[keep]))
    assert np.array_equal(bits(res["pvalue"]), bits(out5[2][iu, ju][keep]))
    assert res["n_edges"] == res["n_rejected"] == keep.sum() and res["n_tests"] == tri.size
    assert adj["n_rejected"].tolist() == [keep.sum(), tri.size] and adj["n_na"] == 0
    assert adj["n_table"] == len(adj["table_p"]) == len(np.unique(tri))
    assert np.array_equal(bits(adj["table_p"]), bits(np.unique(tri)))


def test_refusals_leave_outputs_and_context_untouched(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.pairs(X)                                   # a prepared matrix and a pair list to keep
    L = _lib.lib()
    E_INVALID = -1
    big = np.zeros((1, 65536), order="F")

    def call(Xa, method, alphas, max_table, **kw):
        table = np.full((2, 50), 123.25)
        rc, outs, mx, rc5 = _raw_call(hip_ctx, Xa, method, alphas, max_table, table, **kw)
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == E_INVALID, rc
        assert msg and b"padjust:" in msg, msg
        assert all(np.all(v == (123.25 if v.dtype == np.float64 else -7)) for v in outs.values())
        assert np.all(table == 123.25) and mx[0] == 55.5 and np.all(rc5 == -9)
        assert hip_ctx.num_pairs() == S * (S - 1) // 2    # the refused call touched nothing
        return msg.decode()

    ok = np.array([0.05, 0.5])
    assert "method 7" in call(X, 7, ok, 50)
    assert "method -1" in call(X, -1, ok, 50)
    assert "ICIKT_ADJUST_MAX_ALPHA" in call(X, 3, ok, 50, n_alpha=0)
    assert "ICIKT_ADJUST_MAX_ALPHA" in call(X, 3, np.full(17, 0.5), 50)
    assert "alpha[1]" in call(X, 3, np.array([0.5, np.nan]), 50)
    assert "alpha[0] = -0.1" in call(X, 3, np.array([-0.1]), 50)
    assert "alpha[2] = 1.5" in call(X, 3, np.array([0.0, 1.0, 1.5]), 50)
    assert "max_table" in call(X, 3, ok, -1)
    assert "null alpha" in call(X, 3, ok, 50, null="alpha")
    for name in ("n_tests", "n_rejected", "p_cutoff", "n_table", "table"):
        assert f"null output ({name})" in call(X, 3, ok, 50, null=name)
    assert "ICIKT_TOPK_MAX_SAMPLES" in call(big, 3, ok, 50)
    assert "perspective" in call(X, 3, ok, 50, perspective=7)
    with pytest.raises(_lib.IciktError, match="padjust: method"):
        hip_ctx.padjust(X, "BY", (0.05,))
    with pytest.raises(_lib.IciktError, match=r"padjust: alpha\[0\]"):
        hip_ctx.padjust(X, "BH", (2.0,))
    with pytest.raises(_lib.IciktError, match="padjust: perspective"):
        hip_ctx.padjust(X, "BH", (0.05,), perspective="sideways")
    out, _cnt, rsn = hip_ctx.pairs(X)                  # and the next ordinary call succeeds
    assert out.shape == (S * (S - 1) // 2, 4) and np.all(rsn == 0)


def test_state_after_a_successful_call(hip_ctx):
    S, n = 8, 30
    X = _continuous(S, n)
    hip_ctx.pairs(X)
    got = hip_ctx.padjust(X, "hochberg", (0.05, 1.0), 100)
    assert hip_ctx.num_pairs() == -1
    rc = _lib.lib().icikt_run_dev(hip_ctx._h, 1, 0, 0, 0, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0))
    assert rc == -5, rc                                # ICIKT_E_STATE: nothing prepared
    assert got[0].tolist() == [28, 0] and got[1][1] == 28
    # one column: no pair, no test -- a call, not an error
    one = hip_ctx.padjust(X[:, :1], "BH", (0.05, 1.0), 100)
    assert one[0].tolist() == [0, 0] and one[1].tolist() == [0, 0] and np.all(bits(one[2]) == NA_REAL_BITS)
    assert one[4] == 0 and one[3].shape == (2, 0) and one[5] == -np.inf
    out, _cnt, _rsn = hip_ctx.pairs(X)
    assert out.shape[0] == S * (S - 1) // 2


def test_timing_flag_accounts_the_kernels_under_the_epilogue(hip_ctx):
    S, n = 65, 40
    X = _continuous(S, n)
    hip_ctx.reset_timers()
    hip_ctx.padjust(X, "BH", ALPHAS, 100, flags=_lib.FLAG_TIMING)
    ms, launches = hip_ctx.kernel_ms(_lib.K_EPILOGUE)
    print("epilogue ms", ms, "timed intervals", launches)
    assert ms > 0 and launches >= 2                    # the block's fold, and the sort / adjust / table behind it
    hip_ctx.reset_timers()
