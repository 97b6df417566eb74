"""The grid caps of the grid-strided diagnostics and cor_fast kernels, restated from the host code (test infrastructure
only), and vectorised cor_fast references for pair lists too long for tests/cor_checker.py's per-pair loop.

Past its cap a workgroup (or wave, or y-block) handles several columns or pairs; the later rounds reuse the LDS,
per-block scratch and scan carries of the round before.  Keep these formulas in step with:
- diag_col_blocks:     icikt_capi_diag.cpp, diag_col_pass()        (k_diag_col, 16 bytes of scratch per padded row)
- cor_prep_blocks:     icikt_capi_cor.cpp, icikt_cor_pairs_f64()  prep_blocks (k_cor_prep, 12 bytes per padded row)
- spearman_pw_blocks:  icikt_capi_cor.cpp, icikt_cor_pairs_f64()  pw_blocks (k_cor_spearman_pw, 2 n + 1 int32 per block)
- cor_dots_waves:      icikt_cor.hip, launch_cor_dots()       (k_cor_dots, 4 waves per block, at most 65 536 blocks)
- gather_y_blocks:     icikt_diag.hip, launch_diag_gather()   (k_diag_gather, y-grid)
- complete_chunk:      icikt_capi.cpp, icikt_pairs_complete_in()  chunk (pairs per chunk: 1.5 GiB of masked columns)
- mask_pairs_y_blocks: icikt_epilogue.hip, launch_mask_pairs()    (k_mask_pairs, y-grid: one y-block per pair of the chunk)"""
import numpy as np
from scipy import special, stats

BUDGET = 1 << 29


def np2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def diag_col_blocks(n, S):
    return max(1, min(S, 2048, max(1, BUDGET // (np2(n) * 16))))


def cor_prep_blocks(n, S):
    return max(1, min(S, 2048, max(1, BUDGET // (np2(n) * 12))))


def spearman_pw_blocks(n, P):
    return max(1, min(P, 4096, max(1, BUDGET // ((2 * n + 1) * 4))))


def cor_dots_waves(P):
    return 4 * min((P + 3) // 4, 65536)


def gather_y_blocks(n_cols):
    return min(n_cols, 65535)


def complete_chunk(n):
    return max(1, (3 << 29) // max(16 * n, 16))


def mask_pairs_y_blocks(m):
    return min(m, 65535)


# ---- vectorised cor_fast references (pair batches) -------------------------------------------------------------------

def _t_pvalue_two_sided(t, df):
    t, df = np.asarray(t, float), np.asarray(df, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        t2 = t * t
        near = 0.5 * special.betaincc(0.5, df / 2, t2 / (df + t2))
        far = 0.5 * special.betainc(df / 2, 0.5, df / (df + t2))
    tail = np.where(np.isinf(t), 0.0, np.where(t2 < df, near, far))
    return np.where(np.isnan(t) | ~(df > 0), np.nan, 2 * tail)


def pearson_pairs(X, pi, pj, pairwise, batch=4096):
    """(rho, two-sided p, n_values) of Pearson pairs as tests/cor_checker.check_pairs computes them (two-pass centred
    sums over the jointly present rows; NaN below 3 rows, for a constant side or a non-finite value)."""
    P = len(pi)
    out = np.full((P, 3), np.nan)
    for b0 in range(0, P, batch):
        i, j = pi[b0:b0 + batch], pj[b0:b0 + batch]
        x, y = X[:, i], X[:, j]
        ok = ~np.isnan(x) & ~np.isnan(y)
        m = ok.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            xz, yz = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
            fin = (np.isfinite(xz) & np.isfinite(yz)).all(axis=0)
            mx, my = xz.sum(axis=0) / m, yz.sum(axis=0) / m
            xc, yc = np.where(ok, x - mx, 0.0), np.where(ok, y - my, 0.0)
            const = (np.where(ok, x, np.inf).min(axis=0) == np.where(ok, x, -np.inf).max(axis=0)) | \
                    (np.where(ok, y, np.inf).min(axis=0) == np.where(ok, y, -np.inf).max(axis=0))
            rho = np.clip((xc * yc).sum(axis=0) / np.sqrt((xc * xc).sum(axis=0) * (yc * yc).sum(axis=0)), -1, 1)
            rho = np.where((m < 3) | const | ~fin, np.nan, rho)
            t = np.sqrt(m - 2.0) * rho / np.sqrt(1 - rho * rho)
        out[b0:b0 + batch, 0] = rho
        out[b0:b0 + batch, 1] = _t_pvalue_two_sided(t, m - 2.0)
        out[b0:b0 + batch, 2] = m
    return out


def spearman_dense_pairs(X, pi, pj):
    """(rho, two-sided p, n) of Spearman pairs without NA at n >= 1290 rows (t approximation): integer sums of the
    centred doubled ranks, one rounding of sxy / sqrt(sxx syy)."""
    n = X.shape[0]
    assert n >= 1290 and not np.isnan(X).any()
    R = (2 * stats.rankdata(X, axis=0)).astype(np.int64) - (n + 1)
    ss = (R * R).sum(axis=0)
    sxy = np.array([int(R[:, a] @ R[:, b]) for a, b in zip(pi, pj)], dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.clip(sxy / np.sqrt(ss[pi].astype(float) * ss[pj].astype(float)), -1, 1)
        t = rho / np.sqrt((1 - rho * rho) / (n - 2))
    out = np.empty((len(pi), 3))
    out[:, 0], out[:, 1], out[:, 2] = rho, _t_pvalue_two_sided(t, n - 2.0), n
    return out


def assert_pairs(got, want, label=""):
    """cor_fast's comparison (tests/test_gpu_cor_fast._compare): rho |d| <= 1e-12, n_values exact, p |d| <= 1e-10 and
    <= 1e-8 relative where p >= 1e-290."""
    rho, pv, nv = got[:, 0], got[:, 1], got[:, 2]
    d = np.abs(rho - want[:, 0])
    bad = ~((d <= 1e-12) | (np.isnan(rho) & np.isnan(want[:, 0])))
    assert not bad.any(), f"{label} rho: rows {np.flatnonzero(bad)[:8].tolist()}, max |d| {np.nanmax(d[bad])!r}"
    np.testing.assert_array_equal(nv, want[:, 2], err_msg=label)
    wp = want[:, 1]
    assert np.array_equal(np.isnan(pv), np.isnan(wp)), label
    ok = ~np.isnan(wp)
    np.testing.assert_allclose(pv[ok], wp[ok], atol=1e-10, rtol=0, err_msg=label)
    big = ok & (wp >= 1e-290)
    np.testing.assert_allclose(pv[big], wp[big], rtol=1e-8, atol=0, err_msg=label)


def combn(S):
    i, j = np.triu_indices(S, k=1)
    return i.astype(np.int32), j.astype(np.int32)


def later_round_sample(P, first, rng, k):
    """Every index at or past `first` (handled in a later round) and k from the first round."""
    head = rng.choice(first, size=min(k, first), replace=False) if first else np.zeros(0, np.int64)
    return np.sort(np.concatenate([head, np.arange(first, P)])).astype(np.int64)
