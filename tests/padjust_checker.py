"""Brute-force statement of icikt_padjust_f64's contract, from a full S x S p-value matrix (what Context.matrix or the
CPU oracle returns): the triangle, NaN dropped, sorted, the four formulas of R's p.adjust applied literally -- one IEEE
double operation at a time --, and from the adjusted values every output of the entry, table included.  Plain numpy."""
import numpy as np

NA_REAL_BITS = np.uint64(0x7FF00000000007A2)   # R's NA_real_
METHODS = ("bonferroni", "holm", "hochberg", "BH")
ALPHAS = (0.0, 0.01, 0.05, 0.5, 1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def adjust_sorted(p, method):
    """p: the m p-values ascending.  R's p.adjust(p, method) in that order."""
    p = np.asarray(p, dtype=np.float64)
    m = p.shape[0]
    adj = np.empty(m, dtype=np.float64)
    if method == "bonferroni":
        for i in range(m):
            adj[i] = float(m) * p[i]
    elif method == "holm":
        run = -np.inf
        for i in range(m):                       # j = i + 1: (m + 1 - j) p(j), a running maximum
            run = max(run, float(m - i) * p[i])
            adj[i] = run
    elif method == "hochberg":
        run = np.inf
        for i in range(m - 1, -1, -1):           # a running minimum from the right
            run = min(run, float(m - i) * p[i])
            adj[i] = run
    elif method == "BH":
        run = np.inf
        for i in range(m - 1, -1, -1):
            q = float(m) / float(i + 1)          # the quotient is rounded first, then the product
            run = min(run, q * p[i])
            adj[i] = run
    else:
        raise ValueError(method)
    return np.minimum(1.0, adj)


def adjust_sorted_fast(p, method):
    """adjust_sorted in vector operations (the same IEEE operations element by element), for the large cases."""
    p = np.asarray(p, dtype=np.float64)
    m = p.shape[0]
    left = np.arange(m, 0, -1).astype(np.float64)        # m + 1 - j
    if method == "bonferroni":
        adj = float(m) * p
    elif method == "holm":
        adj = np.maximum.accumulate(left * p)
    elif method == "hochberg":
        adj = np.minimum.accumulate((left * p)[::-1])[::-1]
    elif method == "BH":
        adj = np.minimum.accumulate(((float(m) / np.arange(1, m + 1).astype(np.float64)) * p)[::-1])[::-1]
    else:
        raise ValueError(method)
    return np.minimum(1.0, adj) if m else adj


def sorted_tests(pvalue_matrix):
    """(the p-values of the tests ascending, a zero as +0; n_na: the other pairs of the triangle)"""
    pv = np.asarray(pvalue_matrix, dtype=np.float64)
    tri = pv[np.triu_indices(pv.shape[0], k=1)]
    p = np.sort(tri[~np.isnan(tri)] + 0.0)
    return p, int(tri.shape[0] - p.shape[0])


def outputs_from_sorted(p, n_na, method, alphas=ALPHAS, fast=True):
    adj = (adjust_sorted_fast if fast else adjust_sorted)(p, method)
    m = p.shape[0]
    n_rejected = np.array([int(np.sum(adj <= a)) for a in alphas], dtype=np.int64)
    p_cutoff = np.empty(len(alphas), dtype=np.float64)
    for a, n in enumerate(n_rejected):
        if n > 0:
            p_cutoff[a] = p[n - 1]
        else:
            p_cutoff.view(np.uint64)[a] = NA_REAL_BITS
    most = int(n_rejected.max()) if len(alphas) else 0
    first = np.ones(most, dtype=bool)                   # position i opens a run: i == 0 or p[i] != p[i - 1]
    first[1:] = p[1:most] != p[:max(most - 1, 0)]
    table_p, table_adj = p[:most][first], adj[:most][first]
    return {"n_tests": np.array([m, n_na], dtype=np.int64), "n_rejected": n_rejected, "p_cutoff": p_cutoff,
            "table_p": np.array(table_p, dtype=np.float64), "table_adjusted": np.array(table_adj, dtype=np.float64),
            "n_table": len(table_p), "sorted_p": p, "adjusted": adj}


def brute_padjust(pvalue_matrix, method, alphas=ALPHAS, fast=True):
    """Every output of icikt_padjust_f64 (the whole table: n_table entries), plus the sorted p-values and their
    adjusted values."""
    p, n_na = sorted_tests(pvalue_matrix)
    return outputs_from_sorted(p, n_na, method, alphas, fast)
