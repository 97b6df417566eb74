"""The grid-strided diagnostics and cor_fast kernels past their launch caps (tests/launch_caps.py), on the MI355X: every
shape here makes a workgroup, wave or y-block take a second round, and asserts so first.  Diagnostics are compared bit
for bit with tests/diag_checker.py; cor_fast as tests/test_gpu_cor_fast.py compares it.  Every column or pair of a
later round is checked, plus a sample of the first; the radix-select rows straddle each 4-bit digit boundary of the
doubled ranks."""
import numpy as np
import pytest

from tests import diag_checker as dc
from tests import launch_caps as lc
from tests.cor_checker import check_pairs

pytestmark = pytest.mark.gpu


def censored(rng, n, S, frac=0.15, ties=False):
    X = rng.integers(0, 9, size=(n, S)).astype(np.float64) if ties else rng.lognormal(3, 1, size=(n, S))
    X[rng.random((n, S)) < frac] = np.nan
    X[rng.random((n, S)) < 0.03] = 0.0
    return np.asfortranarray(X)


def cor_matrix(rng, n, S, na=0.0):
    X = rng.normal(size=(n, S)) + 0.3 * rng.normal(size=(n, 1))
    if na:
        X[rng.random(X.shape) < na] = np.nan
    return np.asfortranarray(X)


def run_diag(ctx, X, gna, cls, n_class, rank_cols, label):
    for na_rm in (False, True):
        dc.assert_col_medians(ctx.col_medians(X, na_rm, global_na=gna), X, na_rm, gna, label)
    dc.assert_censor(ctx.censor_counts(X, gna, cls, n_class, want_medians=True), X, gna, cls, n_class, label)
    if rank_cols is not None:
        dc.assert_rank_order(ctx.rank_order(X, gna, rank_cols), X, gna, rank_cols, label)


# ---- diagnostics -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,S,n_rank", [(131073, 129, 129), (131073, 190, 150), (65537, 257, 257), (65537, 300, 280)])
def test_diag_long_columns(hip_ctx, n, S, n_rank):
    """np2 = 2^18 (128 blocks) and 2^17 (256 blocks): one column past the cap, and a partial last round."""
    cap = lc.diag_col_blocks(n, S)
    assert cap == (128 if n > 65536 * 2 else 256) and S > cap and n_rank > lc.diag_col_blocks(n, n_rank)
    rng = np.random.default_rng(n + S)
    X = censored(rng, n, S, ties=S % 2 == 0)
    X[:, S - 1] = np.nan                      # an all-missing column in the last round
    X[n // 3, :] = np.nan
    cls = np.arange(S) % 3
    rank_cols = np.arange(S - n_rank, S, dtype=np.int32)   # consecutive: the in-place route
    run_diag(hip_ctx, X, dc.DEFAULT_NA, cls, 3, rank_cols, f"{n}x{S}")


@pytest.mark.parametrize("n,S", [(4, 2049), (40, 2100), (17, 2049)])
def test_diag_wide_and_short(hip_ctx, n, S):
    """More than 2 048 columns: the fixed cap.  Several hundred classes, some empty, n_class above the largest used;
    rank_order on a class of non-consecutive columns (gathered on the host) past the cap."""
    assert S > lc.diag_col_blocks(n, S) == 2048
    rng = np.random.default_rng(S + n)
    X = censored(rng, n, S, frac=0.25, ties=n == 17)
    X[:, 2048] = np.nan
    X[:, 7] = np.inf
    cls = rng.integers(0, 350, size=S)
    cls[cls == 100] = 101                     # empty classes: 100 and 350 .. 399
    run_diag(hip_ctx, X, (np.nan, np.inf, 0.0, -0.0, 5.0), cls, 400, None, f"{n}x{S}")
    cols = rng.permutation(S).astype(np.int32)       # every column, out of order
    assert len(cols) > lc.diag_col_blocks(n, len(cols))
    dc.assert_rank_order(hip_ctx.rank_order(X, dc.DEFAULT_NA, cols), X, dc.DEFAULT_NA, cols, f"{n}x{S} gathered")


def test_gather_y_stride(hip_ctx):
    """rank_order on one class of 65 537 columns: the gathers' y-grid (65 535) strides twice; original / ordered
    bitwise, missing cells as NA."""
    n, S = 6, 65537
    assert S > lc.gather_y_blocks(S) and S > lc.diag_col_blocks(n, S)
    rng = np.random.default_rng(65537)
    X = censored(rng, n, S, frac=0.3)
    X[:, 65535:] = np.where(rng.random((n, 2)) < 0.5, np.nan, -0.0)   # the second y-round's columns
    X[2, :] = np.nan                                                    # a dropped row
    cols = np.arange(S, dtype=np.int32)
    got = hip_ctx.rank_order(X, dc.DEFAULT_NA, cols)
    ref = dc.assert_rank_order(got, X, dc.DEFAULT_NA, cols, "65537 columns")
    assert ref["n_kept"] == n - 1
    run_diag(hip_ctx, X, dc.DEFAULT_NA, rng.integers(0, 5, size=S), 5, None, "65537 columns")


# ---- cor_fast ----------------------------------------------------------------------------------------------------------

def _check_cor(ctx, X, pi, pj, method, pairwise, sel, label, exact_k=0):
    got, _rsn = ctx.cor_pairs(X, pi, pj, method, pairwise)
    want, _ = check_pairs(X, pi[sel], pj[sel], method, pairwise)
    lc.assert_pairs(got[sel], want, label)
    if exact_k and method == "pearson":
        ex, _ = check_pairs(X, pi[sel[:exact_k]], pj[sel[:exact_k]], method, pairwise, exact=True)
        lc.assert_pairs(got[sel[:exact_k]], ex, label + " exact")
    return got


@pytest.mark.parametrize("n,S", [(131073, 172), (40, 2050)])
def test_cor_prep_past_cap(hip_ctx, n, S):
    """k_cor_prep past its cap (170 blocks at np2 = 2^18, 2 048 at short n), Pearson and Spearman, dense and pairwise:
    every pair with a column of the later round, and a sample of the others."""
    cap = lc.cor_prep_blocks(n, S)
    assert cap == (170 if n > 65536 else 2048) and S > cap
    rng = np.random.default_rng(n * 3 + S)
    late = np.arange(cap, S)
    others = rng.choice(cap, size=30 if n > 1000 else 400, replace=False)
    pi = np.concatenate([np.repeat(others, len(late)), np.full(len(late) - 1, late[0])]).astype(np.int32)
    pj = np.concatenate([np.tile(late, len(others)), late[1:]]).astype(np.int32)
    ei, ej = rng.choice(cap, size=(2, 20))
    keep = ei != ej
    pi, pj = np.concatenate([pi, ei[keep]]).astype(np.int32), np.concatenate([pj, ej[keep]]).astype(np.int32)
    sel = np.arange(len(pi))
    for na in (0.0, 0.1):
        X = cor_matrix(rng, n, S, na)
        for method in ("pearson", "spearman"):
            _check_cor(hip_ctx, X, pi, pj, method, na > 0, sel, f"{n}x{S} {method} na={na}", exact_k=8)


def test_cor_dots_past_wave_cap(hip_ctx):
    """k_cor_dots with more pairs than its 262 144 waves: pairwise Pearson on 800 columns x 64 rows with NA, and a
    shuffled (non-combn) list on dense data, Pearson and Spearman (the dense branch)."""
    n, S = 64, 800
    pi, pj = lc.combn(S)
    P = len(pi)
    waves = lc.cor_dots_waves(P)
    assert P > waves == 262144
    rng = np.random.default_rng(800)
    sel = lc.later_round_sample(P, waves, rng, 3000)
    X = cor_matrix(rng, n, S, 0.1)
    X[:, 5] = np.where(np.arange(n) < 62, np.nan, X[:, 5])        # 2 rows: NA with everyone
    got, _ = hip_ctx.cor_pairs(X, pi, pj, "pearson", True)
    lc.assert_pairs(got[sel], lc.pearson_pairs(X, pi[sel], pj[sel], True), "pairwise pearson")
    ex = sel[-200:]
    want, _ = check_pairs(X, pi[ex], pj[ex], "pearson", True, exact=True)
    lc.assert_pairs(got[ex], want, "pairwise pearson exact")
    perm = rng.permutation(P)
    qi, qj = pj[perm].copy(), pi[perm].copy()                    # not combn: swapped sides, shuffled
    Xd = cor_matrix(rng, n, S)
    got, _ = hip_ctx.cor_pairs(Xd, qi, qj, "pearson", False)
    lc.assert_pairs(got[sel], lc.pearson_pairs(Xd, qi[sel], qj[sel], False), "dense pearson list")
    got, _ = hip_ctx.cor_pairs(Xd, qi, qj, "spearman", False)
    sub = sel[-1500:]
    want, _ = check_pairs(Xd, qi[sub], qj[sub], "spearman", False)
    lc.assert_pairs(got[sub], want, "dense spearman list")


def test_cor_spearman_pw_long_columns(hip_ctx):
    """k_cor_spearman_pw at n = 150 000: 447 blocks of 2 n + 1 scratch, 500 pairs."""
    n, S = 150000, 40
    rng = np.random.default_rng(150000)
    pi, pj = lc.combn(S)
    pick = np.sort(rng.choice(len(pi), size=500, replace=False))
    pi, pj = pi[pick], pj[pick]
    cap = lc.spearman_pw_blocks(n, len(pi))
    assert cap == 447 and len(pi) > cap
    X = cor_matrix(rng, n, S, 0.1)
    X[:, 3] = np.round(X[:, 3] * 3)                           # ties
    sel = lc.later_round_sample(len(pi), cap, rng, 15)
    _check_cor(hip_ctx, X, pi, pj, "spearman", True, sel, "spearman pairwise n=150000")


# ---- radix select of the median ranks ----------------------------------------------------------------------------------

BOUNDARIES = [0x10, 0x100, 0x1000, 0x10000, 0x80000]


def _radix_matrix(rng, n, c):
    """n x c permutation-valued columns (value v: doubled rank 2 v + 2) with probe rows whose middle doubled ranks sit
    at each digit boundary B below 2 n: equal, adjacent within a digit, and split across (B - 1 | B).  Odd doubled
    ranks come from two-row ties; a few columns hold missing cells (their values' ranks shift by 2 k)."""
    X = np.empty((n, c))
    for j in range(c):
        X[:, j] = rng.permutation(n)
    inv = np.argsort(X, axis=0)
    probes, row = [], 7

    def place(j, r, D):        # doubled rank D (even) at row r of column j
        v = D // 2 - 1
        s = inv[v, j]
        X[r, j], X[s, j] = X[s, j], X[r, j]
        inv[int(X[r, j]), j], inv[int(X[s, j]), j] = r, s

    ties, top = [], False
    for B in [b for b in BOUNDARIES if b <= 2 * n]:
        pairs = [(B, B), (B - 2, B)] if c % 2 else [(B - 2, B), (B, B)]
        for lo, hi in pairs + [(B - 1, B + 2), (B - 2, B + 2)]:
            if hi > 2 * n or (hi == 2 * n and top):   # one row only can hold a column's largest rank above its median
                continue
            top = top or hi == 2 * n
            r = row
            row += 97
            mid = (c - 1) // 2
            q = len(probes)
            for j in range(c):
                jj = (j + q) % c                # each probe's middle in other columns than the last one's
                if j < mid:                     # below: distinct small values per probe near the low boundaries
                    D = 2 * (1 + q % (lo // 2 - 2)) if lo < 64 else 2 * int(rng.integers(lo // 4, lo // 2))
                elif j > mid + (c % 2 == 0):    # above
                    D = 2 * int(rng.integers(min(hi // 2 + 1, n), n + 1))
                else:
                    D = lo if j == mid else hi
                if D % 2:                       # odd: values w, w + 1 tie at D = 2 w + 3
                    w = (D - 3) // 2
                    place(jj, r, 2 * w + 2)
                    ties.append((jj, w))
                else:
                    place(jj, r, D)
            probes.append((r, B))
    for j, w in ties:
        X[inv[w + 1, j], j] = w
    for j in range(1, c, 5):                     # missing cells on the rows of the smallest values
        k = int(rng.integers(0, 4))
        X[inv[:k, j], j] = np.nan
    return np.asfortranarray(X), probes


@pytest.mark.parametrize("n,c", [(262144, 1), (262144, 2), (262144, 3), (262144, 16), (262144, 17), (32769, 256),
                                 (32769, 257)])
def test_median_rank_digit_boundaries(hip_ctx, n, c):
    rng = np.random.default_rng(n + c)
    X, probes = _radix_matrix(rng, n, c)
    cols = np.arange(c, dtype=np.int32)
    ref = dc.ref_rank_order(X, (np.nan,), cols)
    # the probe rows really straddle their boundaries: a middle doubled rank at B - 1 or B, or the two around B
    kept = np.flatnonzero(ref["n_na"] < c)
    r2 = np.sort(2 * ref["ranks"], axis=1).astype(np.int64)
    lo_mid, hi_mid = r2[:, (c - 1) // 2], r2[:, c // 2]
    hit = set()
    for r, B in probes:
        k = np.searchsorted(kept, r)
        if k < kept.size and kept[k] == r and (lo_mid[k] < B <= hi_mid[k] or lo_mid[k] in (B - 1, B)):
            hit.add(B)
    assert hit == {b for b in BOUNDARIES if b <= 2 * n}, hit
    assert (lo_mid % 2 == 1).any()                            # a two-row tie in the middle
    if c % 2 == 0:                                            # equal, and distinct middle pairs
        assert (lo_mid == hi_mid).any() and (hi_mid > lo_mid).any()
    got = hip_ctx.rank_order(X, (np.nan,), cols, want_data=False)
    dc.assert_rank_order(got, X, (np.nan,), cols, f"{n}x{c}", ref=ref)


# ---- one context, big -> small -> big ----------------------------------------------------------------------------------

def test_context_reuse_big_small_big(hip_ctx):
    rng = np.random.default_rng(42)
    Xb = censored(rng, 131073, 131)
    Xs = censored(rng, 50, 7)
    Cb = cor_matrix(rng, 131073, 172, 0.05)
    Cs = cor_matrix(rng, 30, 6, 0.1)
    assert Xb.shape[1] > lc.diag_col_blocks(*Xb.shape) and Cb.shape[1] > lc.cor_prep_blocks(*Cb.shape)
    pi_b = np.concatenate([np.arange(20), [170]]).astype(np.int32)
    pj_b = np.concatenate([np.full(20, 171), [171]]).astype(np.int32)
    pi_s, pj_s = lc.combn(6)
    cls_b, cls_s = np.arange(131) % 4, np.arange(7) % 2
    for _ in range(2):
        for X, cls, nc, rank_cols in ((Xb, cls_b, 4, np.arange(131, dtype=np.int32)), (Xs, cls_s, 2, None)):
            for method in ("spearman", "pearson"):
                _check_cor(hip_ctx, Cb, pi_b, pj_b, method, True, np.arange(len(pi_b)), "big cor")
                _check_cor(hip_ctx, Cs, pi_s, pj_s, method, True, np.arange(len(pi_s)), "small cor")
            run_diag(hip_ctx, X, dc.DEFAULT_NA, cls, nc, rank_cols, f"reuse {X.shape}")
        dc.assert_rank_order(hip_ctx.rank_order(Xs, dc.DEFAULT_NA, np.arange(7, dtype=np.int32)), Xs, dc.DEFAULT_NA,
                             np.arange(7), "small rank")
