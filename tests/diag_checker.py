"""CPU checker of the missing-value diagnostics (test infrastructure only): an independent restatement of
icikt_col_medians_f64, icikt_censor_counts_f64 and icikt_rank_order_f64 in numpy, every result exact.

Two forms of each reference.  The slow ones (``*_slow``) walk the columns one at a time with numpy's sort and scipy's
rankdata and are what the fast ones are pinned to (tests/test_diag_checker.py).  The fast ones sort whole column blocks
at once, so that 70 000-column and 131 073 x 200 inputs take seconds:
- ranks: one sort per column block (missing cells last), tie groups from the sorted values, ties averaged;
- missing cells of the kept rows ranked first, in row order;
- row medians of the doubled ranks by np.median, exact because they are integers below 2^20."""
import math

import numpy as np
import scipy.stats as st

NA_BITS = np.uint64(0x7FF00000000007A2)
NAN_BITS = np.uint64(0x7FF8000000000000)
DEFAULT_NA = (math.nan, math.inf, 0.0)
BLOCK_CELLS = 1 << 23     # cells per column block of the fast references


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rule(X, gna):
    """setup_missing_matrix(X, gna) | is.na(X)"""
    miss = np.isnan(X).copy()
    ex = np.zeros(X.shape, dtype=bool)
    for v in gna:
        if math.isnan(v):
            ex |= np.isnan(X)
        elif math.isinf(v):
            ex |= np.isinf(X)
        else:
            ex |= X == v
    return miss | ex, ex


def _blocks(n, S):
    step = max(1, BLOCK_CELLS // max(n, 1))
    for j0 in range(0, S, step):
        yield j0, min(S, j0 + step)


# ---- medians ---------------------------------------------------------------------------------------------------------

def ref_median(v):
    """R's median of the values v (no NA): NA bits when empty, +0 for a zero, NaN bits for mean(-Inf, Inf)."""
    v = np.sort(v)
    m = v.size
    if m == 0:
        return NA_BITS
    if m % 2:
        r = v[m // 2] + 0.0
    else:
        a, b = float(v[m // 2 - 1]), float(v[m // 2])
        with np.errstate(over="ignore", invalid="ignore"):
            s = np.float64(a) + np.float64(b)
        r = 0.5 * s if np.isfinite(s) else (0.5 * a + 0.5 * b if np.isfinite(a) and np.isfinite(b) else s)
        r = r + 0.0
        if np.isnan(r):
            return NAN_BITS
    return np.array([r]).view(np.uint64)[0]


def ref_col_medians_slow(X, miss, na_rm):
    out = np.empty(X.shape[1], dtype=np.uint64)
    for j in range(X.shape[1]):
        out[j] = NA_BITS if (miss[:, j].any() and not na_rm) else ref_median(X[~miss[:, j], j])
    return out


def ref_col_medians(X, miss, na_rm):
    """ref_col_medians_slow over column blocks: one sort of the block, the missing cells sorted last as NaN."""
    n, S = X.shape
    out = np.empty(S, dtype=np.uint64)
    for j0, j1 in _blocks(n, S):
        mk = miss[:, j0:j1]
        Xs = np.sort(np.where(mk, np.nan, X[:, j0:j1]), axis=0)
        cnt = n - mk.sum(axis=0)
        cols = np.arange(j1 - j0)
        h = cnt // 2
        with np.errstate(over="ignore", invalid="ignore"):
            mid = Xs[np.minimum(h, n - 1), cols] if n else np.zeros(j1 - j0)
            a = Xs[np.maximum(h - 1, 0), cols] if n else np.zeros(j1 - j0)
            s = a + mid
            even = np.where(np.isfinite(s), 0.5 * s,
                            np.where(np.isfinite(a) & np.isfinite(mid), 0.5 * a + 0.5 * mid, s))
            r = np.where(cnt % 2 == 1, mid, even) + 0.0
        b = r.view(np.uint64).copy()
        b[np.isnan(r)] = NAN_BITS
        b[cnt == 0] = NA_BITS
        if not na_rm:
            b[cnt < n] = NA_BITS
        out[j0:j1] = b
    return out


# ---- left-censorship counts ------------------------------------------------------------------------------------------

def ref_censor_slow(X, gna, cls, n_class):
    miss, ex = rule(X, gna)
    med = ref_col_medians_slow(X, miss, True).view(np.float64)
    tr, su = np.zeros(n_class, np.int64), np.zeros(n_class, np.int64)
    for k in range(n_class):
        cols = np.flatnonzero(cls == k)
        rows = miss[:, cols].any(axis=1)
        for j in cols:
            if np.isnan(med[j]):
                continue
            x = X[rows, j][~miss[rows, j]]
            tr[k] += x.size
            su[k] += int((x < med[j]).sum())
    return tr, su, int(ex.sum()), med


def ref_censor(X, gna, cls, n_class):
    """(trials, successes, excluded cells, NA-removed medians): per class, over the rows with a missing cell in one of
    the class's columns, the present cells of columns with a median, and those below it."""
    cls = np.asarray(cls)
    miss, ex = rule(X, gna)
    med = ref_col_medians(X, miss, True).view(np.float64)
    tr, su = np.zeros(n_class, np.int64), np.zeros(n_class, np.int64)
    order = np.argsort(cls, kind="stable")
    bounds = np.searchsorted(cls[order], np.arange(n_class + 1))
    for k in range(n_class):
        cols = order[bounds[k]:bounds[k + 1]]
        if cols.size == 0:
            continue
        rows = np.flatnonzero(miss[:, cols].any(axis=1))
        if rows.size == 0:
            continue
        sub, msub = X[np.ix_(rows, cols)], miss[np.ix_(rows, cols)]
        ok = ~msub & ~np.isnan(med[cols])[None, :]
        tr[k] = int(ok.sum())
        with np.errstate(invalid="ignore"):
            su[k] = int((ok & (sub < med[cols][None, :])).sum())
    return tr, su, int(ex.sum()), med


# ---- rank ordering ---------------------------------------------------------------------------------------------------

def _order_result(Xc, miss, kept, med):
    row_order = kept[np.argsort(-med[kept], kind="stable")]
    col_order = np.argsort(-miss[kept].sum(axis=0), kind="stable")
    orig = Xc[kept].copy()
    ob = orig.view(np.uint64)
    ob[miss[kept]] = NA_BITS
    pos = np.searchsorted(kept, row_order)
    return row_order, col_order, orig, orig[pos][:, col_order]


def ref_rank_order_slow(X, gna, cols):
    Xc = X[:, cols]
    miss, _ = rule(Xc, gna)
    n, m = Xc.shape
    n_na = miss.sum(axis=1)
    kept = np.flatnonzero(n_na < m)
    med = np.full(n, np.nan)
    ranks = np.zeros((kept.size, m))
    for j in range(m):
        mk = miss[kept, j]
        k = int(mk.sum())
        ranks[mk, j] = np.arange(1, k + 1)
        if (~mk).any():
            ranks[~mk, j] = k + st.rankdata(Xc[kept, j][~mk] + 0.0, method="average")
    if kept.size:
        med[kept] = np.median(ranks, axis=1)
    row_order, col_order, orig, ordered = _order_result(Xc, miss, kept, med)
    return dict(n_kept=kept.size, n_na=n_na, median_rank=med, row_order=row_order, col_order=col_order,
                original=orig, ordered=ordered, ranks=ranks)


def doubled_ranks(V, mk):
    """2 rank(x, na.last = FALSE) of every column of V (rows x columns) with missing cells mk, as int64: the missing
    cells 2, 4, .. in row order, a value 2 k plus its doubled average rank among the values (a tie group at sorted
    positions [g0, g1) takes g0 + g1 + 1)."""
    n, m = V.shape
    out = np.empty((n, m), dtype=np.int64)
    for j0, j1 in _blocks(n, m):
        v, miss = V[:, j0:j1] + 0.0, mk[:, j0:j1]
        w = j1 - j0
        k = miss.sum(axis=0)
        order = np.argsort(np.where(miss, np.nan, v), axis=0)      # values ascending, the missing cells (NaN) last
        vs = np.take_along_axis(v, order, axis=0)
        pos = np.arange(n)[:, None]
        valid = pos < (n - k)[None, :]
        new = np.ones((n, w), dtype=bool)
        new[1:] = vs[1:] != vs[:-1]
        start = np.maximum.accumulate(np.where(new, pos, 0), axis=0)
        end_new = np.ones((n, w), dtype=bool)
        end_new[:-1] = new[1:]
        end_new |= ~valid | np.vstack([~valid[1:], np.ones((1, w), dtype=bool)])
        end = np.flip(np.minimum.accumulate(np.flip(np.where(end_new, pos + 1, n), axis=0), axis=0), axis=0)
        r2s = 2 * k[None, :] + start + end + 1
        r2 = np.empty((n, w), dtype=np.int64)
        np.put_along_axis(r2, order, r2s, axis=0)
        r2[miss] = (2 * np.cumsum(miss, axis=0))[miss]
        out[:, j0:j1] = r2
    return out


def ref_rank_order(X, gna, cols):
    """rank_order_data of the columns cols of X: the counts, median ranks, orders and gathered cells (ranks: the
    ranks of the kept rows, not doubled)."""
    Xc = X[:, cols]
    miss, _ = rule(Xc, gna)
    n, m = Xc.shape
    n_na = miss.sum(axis=1)
    kept = np.flatnonzero(n_na < m)
    med = np.full(n, np.nan)
    r2 = doubled_ranks(Xc[kept], miss[kept])
    if kept.size:
        med[kept] = np.median(r2, axis=1) / 2
    row_order, col_order, orig, ordered = _order_result(Xc, miss, kept, med)
    return dict(n_kept=kept.size, n_na=n_na, median_rank=med, row_order=row_order, col_order=col_order,
                original=orig, ordered=ordered, ranks=r2 / 2)


# ---- device results against the references ---------------------------------------------------------------------------

def assert_col_medians(got, X, na_rm, gna=None, label=""):
    miss = np.isnan(X) if gna is None else rule(X, gna)[0]
    np.testing.assert_array_equal(bits(got), ref_col_medians(X, miss, na_rm), err_msg=label)


def assert_censor(got, X, gna, cls, n_class, label=""):
    tr, su, nex, med = got
    rtr, rsu, rnex, rmed = ref_censor(X, gna, np.asarray(cls), n_class)
    np.testing.assert_array_equal(tr, rtr, err_msg=label)
    np.testing.assert_array_equal(su, rsu, err_msg=label)
    assert nex == rnex, label
    if med is not None:
        np.testing.assert_array_equal(bits(med), bits(rmed), err_msg=label)


def assert_rank_order(got, X, gna, cols, label="", ref=None):
    ref = ref_rank_order(X, gna, cols) if ref is None else ref
    m = len(cols)
    assert got["n_kept"] == ref["n_kept"], label
    np.testing.assert_array_equal(got["n_na"], ref["n_na"], err_msg=label)
    kept = ref["n_na"] < m
    np.testing.assert_array_equal(bits(got["median_rank"])[kept], bits(ref["median_rank"])[kept], err_msg=label)
    assert (bits(got["median_rank"])[~kept] == NA_BITS).all(), label
    np.testing.assert_array_equal(got["row_order"], ref["row_order"], err_msg=label)
    np.testing.assert_array_equal(got["col_order"], ref["col_order"], err_msg=label)
    if "original" in got:
        np.testing.assert_array_equal(bits(got["original"]), bits(ref["original"]), err_msg=label)
        np.testing.assert_array_equal(bits(got["ordered"]), bits(ref["ordered"]), err_msg=label)
    return ref
