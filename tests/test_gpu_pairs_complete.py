"""icikt_pairs_complete_f64 / _in (kt_fast use = "pairwise.complete.obs") at its caps and chunk edges, on the MI355X.

The entry is the only one that builds its own matrix on the device: k_mask_pairs writes two masked columns per pair of a
chunk, icikt_prepare_dev / icikt_run_dev run on that scratch matrix with the pair list (2k, 2k+1), and each chunk's
results are downloaded at its offset.  Every case asserts first, from the formulas restated in tests/launch_caps.py,
that its shape reaches what it was built for, and compares with tests/complete_checker.py (pinned against scipy and the
O(n^2) enumeration by tests/test_complete_checker.py) as the suite does elsewhere: reasons equal, counts bit-exact where
the reason is 0, the NaN pattern equal with the NA payload on failed pairs, doubles within 1e-10.

Pair lists are seeded random lists over a few dozen columns, repeats and self pairs included: the pair count is free
while the matrix (and the checker's work: once per distinct pair) stays small."""
import warnings

import numpy as np
import pytest

from tests import complete_checker as cc
from tests import launch_caps as lc

pytestmark = pytest.mark.gpu


def _pair_list(rng, S, P):
    return rng.integers(0, S, P).astype(np.int32), rng.integers(0, S, P).astype(np.int32)


def _matrix(rng, n, S, na):
    X = rng.standard_normal((n, S))
    X[:, 1::3] = np.round(X[:, 1::3] * 3)           # a third of the columns rounded to ties
    X[rng.random(X.shape) < na] = np.nan
    return np.asfortranarray(X)


def _same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        if x is None and y is None:
            continue
        assert np.array_equal(x, y, equal_nan=True), f"{what}: output {k} differs ({int((x != y).sum())} entries)"
        if k == 0:
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)), \
                f"{what}: bits of the doubles"


# ---- one shared case per shape: the matrix, the longest list and the checker's answer for it, computed once ------------------

@pytest.fixture(scope="module")
def short_case():
    """n = 24, S = 40, 20 % NA: 131 077 pairs are ONE chunk, three rounds of the mask kernel's y-grid."""
    rng = np.random.default_rng(24)
    X = _matrix(rng, 24, 40, 0.2)
    X[:, 37] = np.where(rng.random(24) < 0.9, np.nan, X[:, 37])      # pairs that keep 0, 1 or 2 rows
    X[:, 38] = np.where(np.isnan(X[:, 38]), np.nan, 4.0)            # constant where present
    X[:, 39] = np.nan
    pi, pj = _pair_list(rng, 40, 131077)
    return X, pi, pj, cc.check_pairs_complete(X, pi, pj)


@pytest.fixture(scope="module")
def chunk_case():
    """n = 4 096 (24 576 pairs per chunk), S = 24, 10 % NA: 49 153 pairs are two full chunks and a chunk of one pair."""
    rng = np.random.default_rng(4096)
    X = _matrix(rng, 4096, 24, 0.1)
    X[:, 5] = np.where(rng.random(4096) < 0.6, np.nan, X[:, 5])
    pi, pj = _pair_list(rng, 24, 49153)
    return X, pi, pj, cc.check_pairs_complete(X, pi, pj)


def _prefix(case, P):
    X, pi, pj, ref = case
    return X, pi[:P], pj[:P], tuple(a[:P] for a in ref)


# ---- past the y cap ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,rounds", [(65535, 1), (65536, 2), (131077, 3)])
def test_one_chunk_past_the_y_grid(hip_ctx, short_case, P, rounds):
    """The mask kernel's y-grid holds 65 535 blocks: a chunk of more pairs takes a second and a third round (the launch
    used to ask for one y-block per pair, whatever their number; the HIP runtime of the day ran that launch too, and the
    entry no longer depends on it).  Every pair is compared."""
    X, pi, pj, ref = _prefix(short_case, P)
    n = X.shape[0]
    assert lc.complete_chunk(n) >= P                                       # one chunk
    assert -(-P // lc.mask_pairs_y_blocks(P)) == rounds
    got = hip_ctx.pairs_complete(X, pi, pj, want_counts=True)
    cc.assert_complete(got, ref, f"P={P}")
    assert (ref[2] != 0).sum() > 100 and (ref[2] == 0).sum() > P // 2     # short columns: failed pairs among healthy ones


# ---- chunk edges ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [24576, 24577, 49153])
@pytest.mark.parametrize("want_counts", [True, False])
def test_chunk_edges(hip_ctx, chunk_case, P, want_counts):
    """P = chunk exactly (one chunk, nothing behind it), chunk + 1 (a last chunk of ONE pair) and 2 chunk + 1: the second
    full chunk has as many pairs as the first, so the entry keeps the first chunk's scratch pair list and task list over a
    freshly prepared matrix, and a third chunk's results land at the offset 2 chunk.  Every pair is compared."""
    X, pi, pj, ref = _prefix(chunk_case, P)
    chunk = lc.complete_chunk(X.shape[0])
    assert chunk == 24576 and P in (chunk, chunk + 1, 2 * chunk + 1)
    got = hip_ctx.pairs_complete(X, pi, pj, want_counts=want_counts)
    assert (got[1] is not None) == want_counts
    cc.assert_complete(got, ref, f"P={P}")
    for first in range(0, P, chunk):                                       # (what a wrong offset would show first)
        last = min(P, first + chunk) - 1
        cc.assert_complete(got, tuple(a[[first, last]] for a in ref), f"chunk at {first}", sel=[first, last])


def test_chunk_edges_without_reasons(hip_ctx, chunk_case):
    """The raw ABI with reasons (and counts) null: 2 chunk + 1 pairs, the same doubles."""
    from icikendalltau_amd import _lib
    L = _lib.lib()
    X, pi, pj, ref = chunk_case
    P = len(pi)
    out = np.full((P, 4), 7.0)
    rc = L.icikt_pairs_complete_f64(hip_ctx._h, X.ctypes.data, X.shape[0], X.shape[1], X.shape[0], pi.ctypes.data,
                                    pj.ctypes.data, P, 0, 0, 0, out.ctypes.data, None, None)
    assert rc == 0, L.icikt_last_error(hip_ctx._h)
    cc.assert_complete((out, None, None), ref, "reasons null")


def test_chunk_edges_long_columns(hip_ctx):
    """n = 50 000 (2 013 pairs per chunk), P = 4 027: two equal chunks and a chunk of one pair on the long-column kernels.
    Compared: the first and last pair of every chunk and a seeded 300 in between."""
    n, S, P = 50000, 8, 4027
    chunk = lc.complete_chunk(n)
    assert chunk == 2013 and P == 2 * chunk + 1
    rng = np.random.default_rng(n)
    X = _matrix(rng, n, S, 0.1)
    pi, pj = _pair_list(rng, S, P)
    sel = np.unique(np.concatenate([[0, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk], rng.choice(P, 300, replace=False)]))
    ref = cc.check_pairs_complete(X, pi[sel], pj[sel])
    got = hip_ctx.pairs_complete(X, pi, pj, want_counts=True)
    cc.assert_complete(got, ref, "n=50000", sel=sel)
    assert np.all(got[2] == 0) and np.all(got[1][:, 1] == 0)               # nothing missing remains after the drop


# ---- pairs that lose their rows ------------------------------------------------------------------------------------------

def _degenerate_list(rng, S):
    """Every pair of the columns, self pairs too, in random order: healthy pairs between the degenerate ones."""
    pi, pj = np.triu_indices(S, k=0)
    flip = rng.random(len(pi)) < 0.5
    pi, pj = np.where(flip, pj, pi), np.where(flip, pi, pj)
    order = rng.permutation(len(pi))
    return pi[order].astype(np.int32), pj[order].astype(np.int32)


@pytest.mark.parametrize("n", [1, 2, 3, 40])
def test_pairs_that_lose_their_rows(hip_ctx, n):
    """Masking leaves 0, 1 or 2 joint rows, or makes one or both sides constant (complete_checker.degenerate_columns): the
    reference's reasons 1, 2, 0 (tau = +-1 without a p-value) and 3, the NA payload on failed pairs; and kt_fast on the
    same matrix gives the same matrices and the same warnings through the HIP engine as through the oracle engine."""
    from icikendalltau_amd import api
    from tests.oracle_engine import OracleEngine
    rng = np.random.default_rng(100 + n)
    X = cc.degenerate_columns(rng, n)
    S = X.shape[1]
    pi, pj = _degenerate_list(rng, S)
    ref = cc.check_pairs_complete(X, pi, pj)
    kinds = set(ref[2].tolist())
    assert kinds >= ({1, 2} if n == 1 else {1, 2, 3} if n == 2 else {0, 1, 2, 3}), kinds
    if n >= 2:                                                             # two joint rows: a tau and no p-value
        two = (ref[2] == 0) & (ref[1][:, 0] == 2)
        assert two.any() and np.isnan(ref[0][two, 1]).all() and np.all(np.abs(ref[0][two, 0]) == 1.0)
    for flags in (0, 1):
        got = hip_ctx.pairs_complete(X, pi, pj, flags=flags, want_counts=True)
        cc.assert_complete(got, ref, f"n={n} flags={flags}")
    names = [f"c{i}" for i in range(S)]
    res = {}
    for label, eng in (("hip", api.HipEngine()), ("oracle", OracleEngine())):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            r = api.kt_fast(X, use="pairwise.complete.obs", colnames=names, engine=eng)
        res[label] = (r["tau"].to_numpy(), r["pvalue"].to_numpy(), sorted(str(x.message) for x in w))
    for k in (0, 1):
        g, o = res["hip"][k], res["oracle"][k]
        assert np.array_equal(np.isnan(g), np.isnan(o)), ("tau", "pvalue")[k]
        assert np.abs(np.where(np.isnan(o), 0.0, g) - np.where(np.isnan(o), 0.0, o)).max(initial=0.0) <= cc.ATOL
    assert res["hip"][2] == res["oracle"][2]
    assert (len(res["oracle"][2]) > 0) == bool((ref[2] > 1).any())


# ---- length regimes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [63, 64, 65, 4097, 10177, 18337, 30656, 30657, 32769, 65535])
def test_length_regimes(hip_ctx, n):
    """Around a step's 64 rows, the half-wave kernels' limits, the whole-wave kernels', two pairs per wave and the longest
    column of the tuned kernels -- on masked columns, which carry a missing block in the SAME rows of both sides (most of
    the column for the pairs of column 5).  64 pairs over 12 columns, every pair compared, flags 0 and EXACT_INT64."""
    from icikendalltau_amd import _lib
    S, P = 12, 64
    rng = np.random.default_rng(n)
    X = _matrix(rng, n, S, 0.1)
    X[:, 5] = np.where(rng.random(n) < 0.6, np.nan, X[:, 5])
    pi, pj = _pair_list(rng, S, P)
    pi[:4], pj[:4] = (5, 0, 5, 4), (1, 5, 5, 4)                            # the 60 % column both ways, self pairs
    assert lc.complete_chunk(n) >= P
    for flags in (0, _lib.FLAG_EXACT_INT64):
        ref = cc.check_pairs_complete(X, pi, pj, int32_compat=not flags)
        got = hip_ctx.pairs_complete(X, pi, pj, flags=flags, want_counts=True)
        cc.assert_complete(got, ref, f"n={n} flags={flags}")
        assert np.all(got[1][:, 1] == 0)


# ---- the planning sample -------------------------------------------------------------------------------------------------

def test_plan_sample_is_the_first_pairs_of_the_chunk(plan_ctx, capfd):
    """The plan's sample (matrix_tied: columns 0 .. 63 of the PREPARED matrix) is here the first 32 pairs of the chunk,
    whatever the caller's columns are.  (a) 32 pairs between continuous columns, then 200 between count-like columns and
    columns of more tie groups than the table the sample sizes; (b) the same list with the tied pairs first.  The two
    orders get opposite verdicts; every pair equals the checker, and per pair the results are bit-identical."""
    from tests.test_gpu_plan_sample import REGIMES, _count_like, _grouped, _ntg, _readback
    n = 17000
    R = REGIMES[n]
    rng = np.random.default_rng(n)
    cont = list(range(0, 8))
    counts = list(range(8, 14))                       # ~1 000 tie groups, most of many rows
    many = list(range(14, 20))                        # more tie groups than any table the sample asks for
    X = rng.standard_normal((n, 20))
    Xc = X[:, cont]
    Xc[rng.random(Xc.shape) < 0.01] = np.nan          # continuous columns with sparse missing values
    X[:, cont] = Xc
    for c in counts:
        X[:, c] = _count_like(rng, n)
    for k, c in enumerate(many):
        X[:, c] = _grouped(rng, n, [2] * (2 * R["cap"] + 100 * k)) if k % 2 == 0 else rng.integers(0, n // 10, n).astype(np.float64)
    late = (counts[-1], many[-1])                     # tied columns with missing values: only behind the sample
    for c in late:
        X[rng.random(n) < 0.05, c] = np.nan
    X = np.asfortranarray(X)
    ci, cj = rng.choice(cont, 32).astype(np.int32), rng.choice(cont, 32).astype(np.int32)
    ti, tj = rng.choice(counts, 200).astype(np.int32), rng.choice(many, 200).astype(np.int32)
    ti[:32], tj[:32] = rng.choice(counts[:-1], 32), rng.choice(many[:-1], 32)
    flip = np.arange(200) % 2 == 1                    # both orientations: each kind streams and is gathered
    ti, tj = np.where(flip, tj, ti).astype(np.int32), np.where(flip, ti, tj).astype(np.int32)
    assert lc.complete_chunk(n) >= 232                # one chunk: one read-back
    tied_sample = np.concatenate([ti[:32], tj[:32]])
    most_tied = max(_ntg(X[:, c]) for c in tied_sample)
    assert most_tied > 2 * R["cap"] > R["hint"] and not np.isnan(X[:, tied_sample]).any()
    res = {}
    for layout, (pi, pj) in (("a", (np.concatenate([ci, ti]), np.concatenate([cj, tj]))),
                             ("b", (np.concatenate([ti, ci]), np.concatenate([tj, cj])))):
        plan_ctx.debug_set_plan({"verbose": "1"})
        capfd.readouterr()
        got = plan_ctx.pairs_complete(X, pi, pj, want_counts=True)
        err = capfd.readouterr().err
        m, most, verdict = _readback(err)
        assert m == 64, err
        if layout == "a":
            assert most < 8 and verdict == R["cont"], err
        else:
            assert most == most_tied and verdict == R["tied"], err
        cc.assert_complete(got, cc.check_pairs_complete(X, pi, pj), f"layout {layout}")
        res[layout] = got
    back = np.concatenate([np.arange(200, 232), np.arange(200)])           # list (a)'s pairs in list (b)
    _same(tuple(a[back] for a in res["b"]), res["a"], "tied pairs first")


# ---- context reuse -------------------------------------------------------------------------------------------------------

def test_context_reuse(chunk_case):
    """One context: a chunked call, a 10-pair call at n = 40, the chunked call again -- bit-identical; then ctx.pairs on
    another matrix equals a fresh context's result (nothing of the scratch matrix or its pair list is left behind)."""
    from icikendalltau_amd import _lib
    X, pi, pj, _ref = _prefix(chunk_case, 24577)
    assert len(pi) > lc.complete_chunk(X.shape[0])
    rng = np.random.default_rng(40)
    Xs = cc.degenerate_columns(rng, 40)
    si, sj = _pair_list(rng, Xs.shape[1], 10)
    Y = _matrix(rng, 700, 9, 0.1)
    ctx, fresh = _lib.Context(0), _lib.Context(0)
    try:
        first = ctx.pairs_complete(X, pi, pj, want_counts=True)
        small = ctx.pairs_complete(Xs, si, sj, want_counts=True)
        cc.assert_complete(small, cc.check_pairs_complete(Xs, si, sj), "10 pairs between chunked calls")
        again = ctx.pairs_complete(X, pi, pj, want_counts=True)
        _same(again, first, "the chunked call again")
        assert ctx.num_pairs() == -1                                        # (include/icikt.h: neither is left behind)
        for persp in ("global", "local"):
            _same(ctx.pairs(Y, perspective=persp), fresh.pairs(Y, perspective=persp), f"pairs after pairs_complete, {persp}")
    finally:
        ctx.close()
        fresh.close()


# ---- wide columns through the front end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65536, 70001])
def test_kt_fast_wide_columns_take_the_host_masked_loop(n):
    """The entry has no path for columns past 65 535 rows; kt_fast sends those through the host-masked loop (eng.pairs takes
    wide columns) instead of raising.  Wide columns are counted in exact integers (tests/test_gpu_parity.py::test_wide_columns),
    so the oracle engine is asked for exact sums too: the reference's 32-bit sums wrap at these lengths."""
    from icikendalltau_amd import _lib, api
    from tests.oracle_engine import OracleEngine
    assert n > _lib.MAX_FEATURES
    rng = np.random.default_rng(n)
    X = _matrix(rng, n, 4, 0.05)
    names = list("abcd")
    g = api.kt_fast(X, use="pairwise.complete.obs", colnames=names)
    o = api.kt_fast(X, use="pairwise.complete.obs", colnames=names, engine=OracleEngine(int32_compat=False))
    for k in ("tau", "pvalue"):
        gv, ov = g[k].to_numpy(), o[k].to_numpy()
        assert np.array_equal(np.isnan(gv), np.isnan(ov)) and not np.isnan(ov[~np.eye(4, dtype=bool)]).any(), k
        assert np.nanmax(np.abs(gv - ov)) <= cc.ATOL, k
