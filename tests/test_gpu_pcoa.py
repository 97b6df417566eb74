"""icikt_pcoa_f64 / _in / _csc on the GPU: the Gower-centred table of PERMANOVA's integers and its largest eigenpairs
(DESIGN.md section 27).

The reference is the brute-force checker (tests/pcoa_checker.py: plain loops, Python ints, int / int) applied to the raw
plane of Context.matrix over all pairs, computed once per data set.  G, the row sums, Q and the pair counts must be
EQUAL, bit for bit; the spectrum is held against numpy.linalg.eigh of that same G within 2 tol |G|_F (one tol is the
solver's criterion, the second covers LAPACK and the rounding of the residual, both about S eps |G|: DESIGN.md section
27).  The shapes are the smallest that reach each part: one pair (S = 2), two (S = 3), a wave's edge (65), two waves
and a tile of rows (130), a workgroup's edge (257) and past it (300, where the default basis of 128 columns is smaller
than the space)."""
import warnings
from fractions import Fraction

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests import designed_tau as dt
from tests import pcoa_checker as pc
from tests.pcoa_checker import bits, na_real
from tests.test_gpu_medians import _continuous

pytestmark = pytest.mark.gpu

SHAPES = [(2, 40), (3, 40), (65, 40), (130, 40), (257, 40), (300, 40)]
TOL = 1e-8
_FULL = {}  # data key -> (raw [S, S], max_taumax, reason_counts) of Context.matrix: computed once
_REF = {}   # data key -> {"n_pairs", "Q", "R", "G", "w" (eigh's eigenvalues, ascending), "frob"}


def _classes3(S, n=40, seed=5):
    """three groups of samples, each a noisy copy of its own profile: three shifted clouds, two large eigenvalues"""
    rng = np.random.default_rng(seed + S)
    profiles = rng.standard_normal((n, 3))
    g = np.arange(S) % 3
    return np.asfortranarray(profiles[:, g] + 0.6 * rng.standard_normal((n, S)))


def _full(ctx, key, X, global_na=None):
    if key not in _FULL:
        out5, _keep, rc5 = ctx.matrix(X, global_na, None, None, "global", "two.sided", False, 0, True, True, want_keep=False)
        tm = out5[3][np.triu_indices(X.shape[1], k=1)]
        tm = tm[~np.isnan(tm)]
        _FULL[key] = (np.array(out5[1]), float(tm.max()) if tm.size else -np.inf, rc5)
    return _FULL[key]


def _reference(ctx, key, X, global_na=None):
    full = _full(ctx, key, X, global_na)
    if key not in _REF:
        n_val, n_na, Q, R, G = pc.brute_gower(full[0])
        ref = {"n_pairs": [n_val, n_na], "Q": Q, "R": R, "G": G}
        if G is not None:
            ref["w"] = np.linalg.eigh(G)[0]
            ref["frob"] = float(np.linalg.norm(G))
        _REF[key] = ref
    return full, _REF[key]


def _assert_integers(got, full, ref):
    n_pairs, Q, R = got[0], got[1], got[2]
    assert n_pairs.dtype == np.int64 and list(n_pairs) == ref["n_pairs"]
    assert isinstance(Q, int) and Q == ref["Q"]
    assert R.dtype == object and list(R) == ref["R"] and sum(int(r) for r in R) == 2 * Q
    assert got[12] == full[1] and np.array_equal(got[13], full[2])


def _assert_spectrum(got, ref, k, tol=TOL):
    """converged; eigenvalues within 2 tol |G|_F of eigh's k largest; recomputed residuals within 2 tol |G|_F;
    |V^T V - I| <= tol; the sign rule"""
    _n, _Q, _R, lam, vec, res, frob, min_ritz, n_basis, n_apply, converged, _G = got[:12]
    G, w = ref["G"], ref["w"]
    F = ref["frob"]
    want = w[::-1][:k]
    recomputed = np.linalg.norm(G @ vec - vec * lam, axis=0)
    print("n_basis", n_basis, "n_apply", n_apply, "converged", converged, "|G|_F", frob, F,
          "max |lambda - eigh| / |G|_F", float(np.abs(lam - want).max() / F), "max residual / |G|_F",
          float(recomputed.max() / F), "reported", float(res.max() / F), "|VtV - I|",
          float(np.abs(vec.T @ vec - np.eye(k)).max()), "min_ritz", min_ritz, "eigh min", w[0])
    assert converged is True
    assert lam.shape == (k,) and vec.shape == (G.shape[0], k) and np.all(np.diff(lam) <= 0)
    assert abs(frob - F) <= 1e-12 * F
    assert np.abs(lam - want).max() <= 2 * tol * F
    assert recomputed.max() <= 2 * tol * F
    assert np.abs(vec.T @ vec - np.eye(k)).max() <= tol
    assert pc.sign_rule_holds(vec)
    assert min_ritz >= w[0] - 2 * tol * F and n_basis <= G.shape[0] and n_apply >= 1


def _same(a, b):
    ok = (np.array_equal(a[0], b[0]) and a[1] == b[1] and list(a[2]) == list(b[2]) and a[8:11] == b[8:11]
          and a[12] == b[12] and np.array_equal(a[13], b[13]) and (a[11] is None) == (b[11] is None))
    for i in (3, 4, 5, 6, 7) + ((11,) if a[11] is not None else ()):
        ok = ok and np.array_equal(bits(a[i]), bits(b[i]))
    return bool(ok)


@pytest.mark.parametrize("S,n", SHAPES)
def test_gower_table_and_integers_bit_for_bit(hip_ctx, S, n):
    X = _continuous(S, n)
    full, ref = _reference(hip_ctx, ("cont", S, n), X)
    got = hip_ctx.pcoa(X, k=min(S - 1, 3), return_gower=True)
    _assert_integers(got, full, ref)
    G = got[11]
    differing = int(np.sum(bits(G) != bits(ref["G"])))
    print("cells", G.size, "differing", differing)
    assert G.shape == (S, S) and differing == 0 and np.array_equal(G, G.T)
    p_pairs, p_Q, _class_q, p_mx, p_rc5 = hip_ctx.permanova(X, None, 1, None)
    assert got[1] == p_Q and np.array_equal(got[0], p_pairs) and got[12] == p_mx and np.array_equal(got[13], p_rc5)
    assert hip_ctx.num_pairs() == -1


@pytest.mark.parametrize("S,k", [(65, 1), (65, 2), (65, 10), (300, 1), (300, 2), (300, 10)])
def test_spectrum_of_class_structured_data_at_the_default_basis(hip_ctx, S, k):
    X = _classes3(S)
    full, ref = _reference(hip_ctx, ("classes3", S), X)
    got = hip_ctx.pcoa(X, k=k, return_gower=True)
    _assert_integers(got, full, ref)
    assert np.array_equal(bits(got[11]), bits(ref["G"]))
    _assert_spectrum(got, ref, k)
    assert got[8] <= min(S, max(8 * k, 128))


@pytest.mark.parametrize("S,n", SHAPES)
def test_spectrum_of_continuous_data_with_a_basis_that_spans_the_space(hip_ctx, S, n):
    X = _continuous(S, n)
    full, ref = _reference(hip_ctx, ("cont", S, n), X)
    k = min(S - 1, 10)
    got = hip_ctx.pcoa(X, k=k, max_basis=S)
    _assert_integers(got, full, ref)
    assert got[11] is None
    _assert_spectrum(got, ref, k)


@pytest.mark.parametrize("S,b", [(2, 1), (65, 16), (130, 17), (257, 32), (300, 33), (300, 64), (513, 10)])
def test_the_apply_kernel_against_numpy(hip_ctx, S, b):
    """every code path of k_pcoa_apply (16, 32 and 64 columns in registers) at its edges, on odd shapes: rows and
    columns that are no multiple of the row tile, of a wave or of the staged chunk (256, 128 and 64 columns).  The bound:
    a row's sum of S products in any order is within S eps sum |g| |v| of the exact one, and numpy's own is too."""
    import torch
    rng = np.random.default_rng(1000 * S + b)
    G = rng.standard_normal((S, S))
    V = rng.standard_normal((b, S))
    dG, dV = torch.from_numpy(G).cuda(), torch.from_numpy(V).cuda()
    dW = torch.full((b, S), -7.0, dtype=torch.float64, device="cuda")
    guard = torch.full((S,), -7.0, dtype=torch.float64, device="cuda")    # (allocated behind dW: must stay as it is)
    torch.cuda.synchronize()
    hip_ctx.pcoa_apply_dev(dG.data_ptr(), dV.data_ptr(), S, b, dW.data_ptr())
    hip_ctx.sync()
    W = dW.cpu().numpy()
    again = torch.empty_like(dW)
    hip_ctx.pcoa_apply_dev(dG.data_ptr(), dV.data_ptr(), S, b, again.data_ptr())
    hip_ctx.sync()
    bound = 2 * S * 2.0 ** -53 * (np.abs(V) @ np.abs(G).T)
    err = np.abs(W - V @ G.T)
    print("largest error / bound", float((err / bound).max()))
    assert np.all(err <= bound) and np.all(guard.cpu().numpy() == -7.0)
    assert np.array_equal(bits(again.cpu().numpy()), bits(W))             # a fixed order: the same bits again
    for bad in ((S, 0), (S, 65), (0, 1)):
        with pytest.raises(_lib.IciktError, match="pcoa_apply"):
            hip_ctx.pcoa_apply_dev(dG.data_ptr(), dV.data_ptr(), bad[0], bad[1], dW.data_ptr())


@pytest.mark.parametrize("k", [17, 40, 64])
def test_wide_blocks_take_the_other_apply_paths(hip_ctx, k):
    S = 130
    X = _classes3(S)
    full, ref = _reference(hip_ctx, ("classes3", S), X)
    got = hip_ctx.pcoa(X, k=k, max_basis=S)
    _assert_integers(got, full, ref)
    _assert_spectrum(got, ref, k)


def test_rank_one_closed_form_ends_by_breakdown(hip_ctx):
    """the swaps family with every sign +1: raw = 1 - 2 |k_a - k_b| / m, so the samples are the points x_a = 2 k_a / m of
    a line, G = (x - x-bar)(x - x-bar)^T up to 2^-48 per cell, lambda_1 = sum (x - x-bar)^2 and
    every other eigenvalue 0"""
    S, n, k = 130, 40, 3
    d = dt.swaps(S, n, seed=3, signs=np.ones(S, dtype=np.int32))
    x = [Fraction(2 * int(p), d.m) for p in d.param]
    mean = sum(x) / S
    dev = [v - mean for v in x]
    lam1 = sum(v * v for v in dev)
    big = max(abs(v) for v in dev)
    first = next(i for i, v in enumerate(dev) if abs(v) == big)
    assert all((v > 0) == (dev[first] > 0) for v in dev if abs(v) == big)     # no tie across the two sides
    sign = 1 if dev[first] > 0 else -1
    res = api.ici_kendalltau_pcoa(d.X, k=k, colnames=[f"s{i}" for i in range(S)], global_na=(np.nan,), return_gower=True)
    F = res["frobenius"]
    bound = TOL * F + S * 2.0 ** -48
    exact_G = np.array([[float(a * b) for b in dev] for a in dev])
    print("lambda_1", float(lam1), "got", res["eigenvalues"], "|G|_F", F, "bound", bound, "n_basis", res["n_basis"],
          "n_apply", res["n_apply"], "max |G - exact|", float(np.abs(res["gower"] - exact_G).max()),
          "max coordinate error", float(np.abs(res["coordinates"][:, 0] - sign * np.array([float(v) for v in dev])).max()))
    assert np.abs(res["gower"] - exact_G).max() <= 2.0 ** -48
    assert abs(F - float(lam1)) <= bound
    assert res["converged"] is True and res["n_basis"] <= 2 * k
    assert abs(res["eigenvalues"][0] - float(lam1)) <= bound
    assert np.abs(res["eigenvalues"][1:]).max() <= bound
    assert np.abs(res["coordinates"][:, 0] - sign * np.array([float(v) for v in dev])).max() <= bound
    assert np.abs(res["coordinates"][:, 1:]).max() <= np.sqrt(bound)          # sqrt of an eigenvalue within the bound of 0
    assert abs(res["total_inertia"] - float(lam1)) <= bound and abs(res["proportion"][0] - 1.0) <= 1e-6
    assert res["n_na"] == 0 and res["max_taumax"] == 1.0


def test_a_basis_too_small_returns_the_best_pairs_and_warns_once(hip_ctx):
    S, n, k = 300, 40, 10
    X = _continuous(S, n)
    full, ref = _reference(hip_ctx, ("cont", S, n), X)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = api.ici_kendalltau_pcoa(X, k=k, max_basis=20, colnames=[f"s{i}" for i in range(S)], global_na=(np.nan,))
    assert sum("has not converged" in str(x.message) for x in w) == 1 and len(w) == 1
    assert res["converged"] is False and res["n_basis"] == 20 and res["n_apply"] == 2
    F = ref["frob"]
    recomputed = np.linalg.norm(ref["G"] @ res["vectors"] - res["vectors"] * res["eigenvalues"], axis=0)
    print("residuals / |G|_F", res["residuals"] / F, "recomputed", recomputed / F)
    assert res["residuals"].max() > TOL * F
    assert np.abs(res["residuals"] - recomputed).max() <= TOL * F
    assert np.abs(res["vectors"].T @ res["vectors"] - np.eye(k)).max() <= TOL and pc.sign_rule_holds(res["vectors"])
    assert res["sums"]["q_total"] == ref["Q"] and res["max_taumax"] == full[1]


@pytest.mark.parametrize("spec", ["tkblock=1000", "tkblock=1"])
def test_block_cuts_give_identical_output(plan_ctx, spec):
    S = 130
    X = _classes3(S)
    want = plan_ctx.pcoa(X, k=10, return_gower=True)
    plan_ctx.debug_set_plan(spec)
    assert _same(plan_ctx.pcoa(X, k=10, return_gower=True), want)


def test_layouts_pinned_memory_and_repeated_calls_give_identical_output(hip_ctx):
    sp = pytest.importorskip("scipy.sparse")
    S, n = 65, 40
    rng = np.random.default_rng(22)
    X = np.asfortranarray(rng.poisson(1.5, (n, S)).astype(np.float64) * rng.integers(1, 50, (n, S)))
    gna = [np.nan, np.inf, 0.0]
    X32 = np.ascontiguousarray(X.astype(np.float32))
    assert np.array_equal(X32.astype(np.float64), X) and _lib.input_view(X32)[2] == _lib.ORDER_ROW
    want = hip_ctx.pcoa(X, k=5, return_gower=True, global_na=gna)
    full, ref = _reference(hip_ctx, "counts", X, gna)
    _assert_integers(want, full, ref)
    assert np.array_equal(bits(want[11]), bits(ref["G"]))
    _assert_spectrum(want, ref, 5)
    assert _same(hip_ctx.pcoa(X, k=5, return_gower=True, global_na=gna), want)            # two calls in a row
    assert _same(hip_ctx.pcoa(X32, k=5, return_gower=True, global_na=gna), want)
    assert _same(hip_ctx.pcoa(sp.csc_matrix(X), k=5, return_gower=True, global_na=gna), want)
    hip_ctx.f64_entries = True
    try:
        assert _same(hip_ctx.pcoa(X, k=5, return_gower=True, global_na=gna), want)        # the _f64 entry
    finally:
        hip_ctx.f64_entries = False
    Xp = _lib.pinned_empty(X.shape, order="F")
    Xp[...] = X
    assert _same(hip_ctx.pcoa(Xp, k=5, return_gower=True, global_na=gna, flags=_lib.FLAG_HOST_PINNED), want)


def test_a_used_context_and_a_caller_stream_equal_a_fresh_context(hip_ctx):
    import torch
    from tests.test_gpu_caller_stream import Lane
    S = 130
    X = _classes3(S)
    big = _classes3(300)
    fresh = _lib.Context(0)
    try:
        want = fresh.pcoa(X, k=10, return_gower=True)
    finally:
        fresh.close()
    for other in (lambda: hip_ctx.hclust(X, "average"), lambda: hip_ctx.permanova(X, None, 1, None),
                  lambda: hip_ctx.pcoa(big, k=12)):
        other()
        assert _same(hip_ctx.pcoa(X, k=10, return_gower=True), want)
    ctx = _lib.Context(0)
    try:
        lane = Lane(ctx, "side")
        with torch.cuda.stream(lane.ts):
            a = torch.ones(1 << 22, device="cuda")
            b = a + a                                                   # the caller's work, ahead of the call
        assert _same(ctx.pcoa(X, k=10, return_gower=True), want)
        with torch.cuda.stream(lane.ts):
            assert float(b[-1]) == 2.0
    finally:
        ctx.close()


def test_an_all_missing_column_makes_every_double_na(hip_ctx):
    S, n, k = 65, 40, 4
    X = _continuous(S, n).copy()
    X[:, 5] = np.nan
    full, ref = _reference(hip_ctx, "cont-na", X)
    assert ref["n_pairs"][1] == S - 1 and ref["G"] is None
    got = hip_ctx.pcoa(X, k=k, return_gower=True)
    _assert_integers(got, full, ref)
    for i in (3, 4, 5, 6, 7, 11):
        assert np.all(bits(got[i]) == bits(na_real())[0]), i
    assert got[8:11] == (0, 0, False) and got[4].shape == (S, k) and got[11].shape == (S, S)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = api.ici_kendalltau_pcoa(X, k=k, colnames=[f"s{i}" for i in range(S)], global_na=(np.nan,))
    assert sum("PCoA needs every pair" in str(x.message) for x in w) == 1 and len(w) == 1
    assert res["n_na"] == S - 1 and list(res["sums"]["row_q"]) == ref["R"] and res["sums"]["q_total"] == ref["Q"]
    for key in ("coordinates", "eigenvalues", "proportion", "vectors", "total_inertia", "residuals", "frobenius", "min_ritz"):
        assert np.all(bits(res[key]) == bits(na_real())[0]), key


def test_refusals_leave_the_outputs_untouched(hip_ctx):
    S, n, k = 70, 40, 3
    X = np.asfortranarray(_continuous(S, n))
    L = _lib.lib()
    start = np.random.default_rng(0).standard_normal((65, S))
    ints = {"n_pairs": np.full(2, -9, dtype=np.int64), "q_total": np.full(2, -9, dtype=np.int64),
            "row_lo": np.full(S, -9, dtype=np.int64), "row_hi": np.full(S, -9, dtype=np.int64)}
    dbls = {"eigenvalues": np.full(65, -9.0), "vectors": np.full(65 * S, -9.0), "residuals": np.full(65, -9.0),
            "frobenius": np.full(1, -9.0), "min_ritz": np.full(1, -9.0)}
    solver = np.full(3, -9, dtype=np.int64)
    gower = np.full(S * S, -9.0)

    def call(k=k, tol=1e-8, max_basis=0, n_samp=S, null=None, start_arg=start, perspective=1):
        ptr = {name: (None if name == null else _lib._ptr(a)) for name, a in {**ints, **dbls, "solver": solver}.items()}
        rc = L.icikt_pcoa_f64(hip_ctx._h, _lib._ptr(X), n, n_samp, n, None, 0, perspective, 0, 0, 0, k, tol, max_basis,
                              _lib._ptr(start_arg), ptr["n_pairs"], ptr["q_total"], ptr["row_lo"], ptr["row_hi"],
                              ptr["eigenvalues"], ptr["vectors"], ptr["residuals"], ptr["frobenius"], ptr["min_ritz"],
                              ptr["solver"], _lib._ptr(gower), None, None)
        msg = L.icikt_last_error(hip_ctx._h)
        assert rc == -1 and msg and msg.startswith(b"pcoa:"), (rc, msg)
        assert all(np.all(a == -9) for a in list(ints.values()) + list(dbls.values()) + [solver, gower])
        return msg.decode()

    assert "k must be in 1 .. min(n_samp - 1, 64)" in call(k=0)
    assert "k must be in 1 .. min(n_samp - 1, 64)" in call(k=65)                       # k <= S - 1 = 69, past the cap
    assert "k must be in 1 .. min(n_samp - 1, 64)" in call(k=40, n_samp=40)            # k = S
    assert "tol must be positive" in call(tol=0.0)
    assert "tol must be positive" in call(tol=float("nan"))
    assert "max_basis must be 0 (the default) or at least k" in call(max_basis=k - 1)
    assert "n_samp must be at least 2" in call(n_samp=1, k=1)
    assert "null start block" in call(start_arg=None)
    for name in list(ints) + list(dbls) + ["solver"]:
        assert f"null output ({name})" in call(null=name)
    assert "perspective" in call(perspective=7)
    for kw, text in (({"k": 0}, "k must be"), ({"k": S}, "k must be"), ({"k": 65}, "k must be"), ({"tol": 0}, "tol must be"),
                     ({"k": 5, "max_basis": 4}, "max_basis must be")):
        with pytest.raises(_lib.IciktError, match=text):
            hip_ctx.pcoa(X, **kw)
    with pytest.raises(_lib.IciktError, match="n_samp must be at least 2"):
        hip_ctx.pcoa(X[:, :1], k=1)
    full, ref = _reference(hip_ctx, ("cont", S, n), X)                   # the next call on the same context is right
    got = hip_ctx.pcoa(X, k=k, max_basis=S, return_gower=True)
    _assert_integers(got, full, ref)
    assert np.array_equal(bits(got[11]), bits(ref["G"]))
    _assert_spectrum(got, ref, k)
    assert hip_ctx.num_pairs() == -1
