"""Brute-force checker of icikt_mantel_f64, in plain loops, Python ints and Fractions.

From a full S x S `raw` matrix (Context.matrix's plane 1, or a designed one) and `other` (S x S or condensed) it makes
the two integer vectors, sums T of the identity and of every permutation, compares the sums as Python ints and takes r
through a 150-digit `decimal` square root.  Nothing of it comes from the library or from icikendalltau_amd.api.

The rule.  P = S (S - 1) / 2 pairs i < j in combn order.  x is 1 - raw of the data, y is `other`.
  spearman   both vectors become doubled average ranks among the P values, ascending in value (for x: ascending 1 - raw,
             that is descending raw, -0 equal to +0): lo + hi + 1 with lo the values below and hi those at or below
  pearson    xv = rint((1.0 - raw) 2^30); yv = rint((y - lo) 2^(31 - e)) with lo, hi the smallest and largest y and
             (m, e) = frexp(hi - lo); every step one IEEE double operation, rounding half to even
T(pi) = sum_{i<j} xv_ij yv_{pi(i) pi(j)}; r = (P T - Sx Sy) / sqrt((P Sxx - Sx^2)(P Syy - Sy^2)), NA when a factor is 0.
A pair whose raw is NaN: nothing is summed (every T and moment 0, n_ge = n_le = 0) and every double is NA.

`brute_mantel(..., loops=True)` is the rule in plain loops; the default takes the same sums with numpy in pieces that
cannot overflow, for the shapes of the GPU tests (tests/test_mantel_host.py holds the two against each other).
"""
import decimal
import math
from fractions import Fraction

import numpy as np

NA_REAL_BITS = 0x7FF00000000007A2   # R's NA_real_


def na_real():
    return float(np.array([NA_REAL_BITS], dtype=np.uint64).view(np.float64)[0])


def bits(a):
    return np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64).view(np.int64)


def condensed(other, S):
    """`other` as the list of its P values in combn order"""
    a = np.asarray(other, dtype=np.float64)
    if a.ndim == 2:
        assert a.shape == (S, S)
        return np.array([a[i, j] for i in range(S) for j in range(i + 1, S)], dtype=np.float64)
    assert a.shape == (S * (S - 1) // 2,)
    return a.copy()


def rank2_loops(values):
    """doubled average ranks, ascending: lo + hi + 1, O(P^2) comparisons of doubles (-0 == +0 as doubles compare)"""
    v = [float(u) for u in values]
    return [sum(1 for u in v if u < w) + sum(1 for u in v if u <= w) + 1 for w in v]


def rank2(values):
    v = np.asarray(values, dtype=np.float64) + 0.0
    asc = np.sort(v)
    return (np.searchsorted(asc, v, "left") + np.searchsorted(asc, v, "right") + 1).astype(np.int64)


def quantise_x(raw_values):
    """xv of raw values without NaN as Python ints: one subtraction in double, then an exact scaling and rint"""
    out = []
    for r in raw_values:
        d = 1.0 - (float(r) + 0.0)
        out.append(int(np.rint(math.ldexp(d, 30))))
    return out


def quantise_y(y):
    y = [float(u) for u in y]
    if not y:
        return []
    lo, hi = min(y), max(y)
    span = hi - lo
    assert math.isfinite(span)
    e = math.frexp(span)[1]
    return [int(np.rint(math.ldexp(u - lo, 31 - e))) for u in y]


def integers(raw, other, method):
    """(xv, yv, n_na): the two integer vectors as int64 arrays in combn order (None, None with an NA pair)"""
    raw = np.asarray(raw, dtype=np.float64)
    S = raw.shape[0]
    iu, ju = np.triu_indices(S, k=1)
    v = raw[iu, ju]
    n_na = int(np.isnan(v).sum())
    if n_na:
        return None, None, n_na
    y = condensed(other, S)
    if method == "spearman":
        return rank2(-(v + 0.0) + 0.0), rank2(y), 0     # ascending 1 - raw is ascending -raw
    return np.array(quantise_x(v), dtype=np.int64), np.array(quantise_y(y), dtype=np.int64), 0


def dot_int(x, y):
    """sum x y of int64 arrays below 2^32 as a Python int: y in 16-bit halves, pieces of 2^14 products below 2^48"""
    total = 0
    for a in range(0, x.shape[0], 1 << 14):
        xs, ys = x[a:a + (1 << 14)], y[a:a + (1 << 14)]
        total += int(np.sum(xs * (ys & 0xFFFF))) + (int(np.sum(xs * (ys >> 16))) << 16)
    return total


def statistic(P, T, sx, sxx, sy, syy):
    """r as a double through a 150-digit square root; None when undefined"""
    vx, vy = P * sxx - sx * sx, P * syy - sy * sy
    if P <= 0 or vx <= 0 or vy <= 0:
        return None
    num = P * T - sx * sy
    with decimal.localcontext() as ctx:
        ctx.prec = 150
        r = decimal.Decimal(num) / (decimal.Decimal(vx) * decimal.Decimal(vy)).sqrt()
        return float(r)


def to_double(v):
    return na_real() if v is None else float(v)


def brute_mantel(raw, other, method, perms, loops=False):
    """A dict of everything icikt_mantel_f64 and the front end return, from `raw` [S, S], `other`, the method and the
    permutations [n_perm, S] of sample indices."""
    raw = np.asarray(raw, dtype=np.float64)
    S = raw.shape[0]
    P = S * (S - 1) // 2
    perms = np.asarray(perms, dtype=np.int64).reshape(-1, S)
    n_perm = perms.shape[0]
    for row in perms:
        assert sorted(row.tolist()) == list(range(S))
    pair_list = [(i, j) for i in range(S) for j in range(i + 1, S)] if loops else None
    if loops:
        vals = [float(raw[i, j]) for i, j in pair_list]
        n_na = sum(1 for u in vals if u != u)
        if n_na == 0:
            y = [float(u) for u in condensed(other, S)]
            if method == "spearman":
                xv, yv = rank2_loops([-(u + 0.0) + 0.0 for u in vals]), rank2_loops(y)
            else:
                xv, yv = quantise_x(vals), quantise_y(y)
    else:
        xv, yv, n_na = integers(raw, other, method)
    T = [0] * (1 + n_perm)
    mom = (0, 0, 0, 0)
    n_ge = n_le = 0
    if n_na == 0:
        labs = [list(range(S))] + [row.tolist() for row in perms]
        if loops:
            table = [[0] * S for _ in range(S)]
            for (i, j), w in zip(pair_list, yv):
                table[i][j] = table[j][i] = int(w)
            for t, pi in enumerate(labs):
                T[t] = sum(int(xw) * table[pi[i]][pi[j]] for (i, j), xw in zip(pair_list, xv))
            mom = (sum(int(u) for u in xv), sum(int(u) ** 2 for u in xv), sum(int(u) for u in yv), sum(int(u) ** 2 for u in yv))
        else:
            iu, ju = np.triu_indices(S, k=1)
            table = np.zeros((S, S), dtype=np.int64)
            table[iu, ju] = yv
            table[ju, iu] = yv
            for t, pi in enumerate(labs):
                pi = np.asarray(pi, dtype=np.int64)
                T[t] = dot_int(xv, table[pi[iu], pi[ju]])
            mom = (int(xv.sum()), dot_int(xv, xv), int(yv.sum()), dot_int(yv, yv))
        n_ge = sum(1 for t in T[1:] if t >= T[0])
        n_le = sum(1 for t in T[1:] if t <= T[0])
    obs = statistic(P, T[0], *mom) if n_na == 0 else None
    stats = [statistic(P, t, *mom) if n_na == 0 else None for t in T[1:]]
    return {
        "n_pairs": np.array([P - n_na, n_na], dtype=np.int64), "T": T, "moments": mom, "n_ge": n_ge, "n_le": n_le,
        "xv": xv if n_na == 0 else None, "yv": yv if n_na == 0 else None,
        "statistic": to_double(obs),
        "pvalue": na_real() if obs is None else float(Fraction(1 + n_ge, 1 + n_perm)),
        "perm_statistic": np.array([to_double(f) for f in stats], dtype=np.float64),
    }


def documented_permutations(S, n_perm, seed, strata=None):
    """The front end's documented contract, written out independently: one default_rng(seed); permutation t is
    rng.permutation(arange(S)); with strata the indices of each stratum (first appearance first) are permuted in place."""
    idx = np.arange(S, dtype=np.int32)
    rng = np.random.default_rng(seed)
    out = []
    order = []
    if strata is not None:
        for v in strata:
            if v not in order:
                order.append(v)
    for _t in range(n_perm):
        if strata is None:
            out.append(rng.permutation(idx))
            continue
        row = idx.copy()
        for v in order:
            ix = np.array([s for s, u in enumerate(strata) if u == v], dtype=np.intp)
            row[ix] = rng.permutation(idx[ix])
        out.append(row)
    return np.array(out, dtype=np.int32).reshape(n_perm, S)
