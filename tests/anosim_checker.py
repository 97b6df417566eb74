"""Brute-force checker of icikt_anosim_f64, in numpy and Python ints.

From a full S x S `raw` matrix (Context.matrix's plane 1, or a designed one) it takes the triangle's valid values,
ranks them, sums the within-class ranks of every labelling by a masked sum over ALL values, compares the statistics as
fractions of Python ints and converts each double once, through `fractions.Fraction`.  Nothing of it comes from the
library or from icikendalltau_amd.api.

The rule.  A pair i < j is a value iff its raw is not NaN; M values.  The dissimilarity is 1 - raw: a value's rank is
its average rank among the M values in DESCENDING raw (-0 equals +0), and r2 = 2 * rank is an integer.  For a labelling
W2 is the sum of r2 over the values whose two samples share a class, nW their count, nB = M - nW, T2 = M (M + 1), and
R = (T2 nW - W2 M) / (nW nB M); undefined when nW = 0 or nB = 0.
"""
from fractions import Fraction

import numpy as np

NA_REAL_BITS = 0x7FF00000000007A2   # R's NA_real_


def na_real():
    return float(np.array([NA_REAL_BITS], dtype=np.uint64).view(np.float64)[0])


def bits(a):
    return np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64).view(np.int64)


def triangle_values(raw):
    """(i, j, value) of the valid pairs in combn order, -0 as +0; (M, n_na)"""
    raw = np.asarray(raw, dtype=np.float64)
    S = raw.shape[0]
    iu, ju = np.triu_indices(S, k=1)
    v = raw[iu, ju]
    ok = ~np.isnan(v)
    return iu[ok], ju[ok], v[ok] + 0.0, int(ok.sum()), int((~ok).sum())


def doubled_ranks(values):
    """r2 of every value: twice its average rank in ascending 1 - raw.  Sort + two searches on -raw: with `below` the
    values of smaller -raw and `upto` those of smaller or equal -raw, the tied run holds the ranks below + 1 .. upto,
    whose mean doubled is below + upto + 1."""
    neg = -(np.asarray(values, dtype=np.float64) + 0.0) + 0.0
    asc = np.sort(neg)
    below = np.searchsorted(asc, neg, side="left").astype(np.int64)
    upto = np.searchsorted(asc, neg, side="right").astype(np.int64)
    return below + upto + 1


def statistic(M, w2, nw):
    """R as a Fraction of Python ints, None when undefined"""
    M, w2, nw = int(M), int(w2), int(nw)
    nb = M - nw
    if nw <= 0 or nb <= 0:
        return None
    return Fraction(M * (M + 1) * nw - w2 * M, nw * nb * M)


def to_double(frac):
    return na_real() if frac is None else float(frac)


def brute_anosim(raw, cls, n_class, perms):
    """A dict of everything icikt_anosim_f64 and the front end return, from `raw` [S, S], the observed class codes
    [S], n_class and the permutations [n_perm, S]."""
    cls = np.asarray(cls, dtype=np.int64)
    S = cls.shape[0]
    perms = np.asarray(perms, dtype=np.int64).reshape(-1, S)
    i, j, v, M, n_na = triangle_values(raw)
    r2 = doubled_ranks(v)
    assert M == 0 or (int(r2.sum()) == M * (M + 1) and r2.min() >= 2 and r2.max() <= 2 * M)
    labs = np.vstack([cls[None, :], perms])
    w2 = np.zeros(labs.shape[0], dtype=np.int64)
    nw = np.zeros(labs.shape[0], dtype=np.int64)
    for q, lab in enumerate(labs):
        within = lab[i] == lab[j]
        w2[q] = int(np.sum(r2[within], dtype=np.int64))
        nw[q] = int(np.sum(within))
    obs = statistic(M, w2[0], nw[0])
    stats = [statistic(M, a, b) for a, b in zip(w2[1:], nw[1:])]
    n_undefined = sum(1 for f in stats if f is None)
    n_ge = 0 if obs is None else sum(1 for f in stats if f is not None and f >= obs)
    class_w2 = np.zeros(n_class, dtype=np.int64)
    class_nw = np.zeros(n_class, dtype=np.int64)
    within = cls[i] == cls[j]
    for c in range(n_class):
        of_c = within & (cls[i] == c)
        class_w2[c] = int(np.sum(r2[of_c], dtype=np.int64))
        class_nw[c] = int(np.sum(of_c))
    n_perm = perms.shape[0]
    W2, nW = int(w2[0]), int(nw[0])
    return {
        "n_pairs": np.array([M, n_na], dtype=np.int64), "w2": w2, "nw": nw, "n_ge": n_ge, "n_undefined": n_undefined,
        "class_w2": class_w2, "class_nw": class_nw, "r2": r2, "i": i, "j": j,
        "statistic": to_double(obs),
        "pvalue": na_real() if obs is None else float(Fraction(1 + n_ge, 1 + n_perm)),
        "perm_statistic": np.array([to_double(f) for f in stats], dtype=np.float64),
        "class_mean_rank": np.array([to_double(Fraction(int(a), 2 * int(b)) if b else None)
                                     for a, b in zip(class_w2, class_nw)], dtype=np.float64),
        "within_mean_rank": to_double(Fraction(W2, 2 * nW) if nW else None),
        "between_mean_rank": to_double(Fraction(M * (M + 1) - W2, 2 * (M - nW)) if M > nW else None),
        "exact": (obs, stats),
    }


def documented_permutations(codes, n_perm, seed, strata=None):
    """The front end's documented contract, written out independently: one default_rng(seed); permutation t is
    rng.permutation(codes); with strata the codes of each stratum (first appearance first) are permuted in place."""
    codes = np.asarray(codes, dtype=np.int32)
    rng = np.random.default_rng(seed)
    out = []
    order = []
    if strata is not None:
        for v in strata:
            if v not in order:
                order.append(v)
    for _t in range(n_perm):
        if strata is None:
            out.append(rng.permutation(codes))
            continue
        row = codes.copy()
        for v in order:
            ix = np.array([s for s, u in enumerate(strata) if u == v], dtype=np.intp)
            row[ix] = rng.permutation(codes[ix])
        out.append(row)
    return np.array(out, dtype=np.int32).reshape(n_perm, codes.shape[0])
