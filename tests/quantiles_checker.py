"""Brute-force statement of icikt_quantiles_f64's contract, from five full S x S matrices (cor, raw, pvalue, taumax,
completeness) and a class index per sample.  Used by the CPU tests of the front end and the GPU tests of the kernels.

Pairs: the upper triangle i < j.  Groups: 0 every pair; with cls also 1 the pairs with cls[i] == cls[j] and 2 the pairs
with cls[i] != cls[j].  A pair whose raw is NA is no value: n_na[g] counts those, n_valid[g] the others.
Order statistics: the valid raw values of a group sorted ascending as x[1..v], a zero counting as +0.  For a prob p,
index = 1 + (v - 1) p in float64, lo = floor(index), hi = ceil(index): order2 holds x[lo] and x[hi].
quantile_raw: R's quantile(type = 7): a = x[lo], b = x[hi], h = index - lo; a when index == lo or a == b, else
(1 - h) a + h b, every operation a float64 operation of its own; a zero as +0.  quantile_cor: the same rule on the cor
cells of the two pairs that supplied a and b.  v = 0: NA_real_ everywhere.
Histogram: numpy.histogram(valid raw, bins=breaks); outside: the values below breaks[0] and above breaks[-1]."""
import math

import numpy as np

NA_REAL_BITS = np.uint64(0x7FF00000000007A2)
PROBS = (0, 1, 0.5, 0.25, 1 / 3, 0.999, 0.5, 0.1)     # unsorted, with a repeat and both ends


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def type7(a, b, index, lo):
    a, b = float(a), float(b)
    if index == lo or a == b:
        return a + 0.0
    h = index - lo
    left = (1.0 - h) * a
    right = h * b
    return (left + right) + 0.0


def group_masks(S, cls):
    """(iu, ju, [mask per group]) over the upper triangle in combn order"""
    iu, ju = np.triu_indices(S, k=1)
    every = np.ones(iu.shape[0], dtype=bool)
    if cls is None:
        return iu, ju, [every]
    cls = np.asarray(cls)
    same = cls[iu] == cls[ju]
    return iu, ju, [every, same, ~same]


def brute_quantiles(out5, cls, probs, breaks):
    """(q2 [2, G, n_probs]: cor, raw; order2 [G, n_probs, 2]; n_valid [G]; n_na [G]; hist [G, n_bins]; outside [G, 2])"""
    cor = np.ascontiguousarray(out5[0], dtype=np.float64)
    raw = np.ascontiguousarray(out5[1], dtype=np.float64)
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    breaks = None if breaks is None else np.asarray(breaks, dtype=np.float64)
    iu, ju, masks = group_masks(raw.shape[0], cls)
    with np.errstate(invalid="ignore"):      # (NA_real_ is a signalling NaN)
        tri_raw, tri_cor = raw[iu, ju] + 0.0, cor[iu, ju] + 0.0
    G, n_probs, n_bins = len(masks), probs.shape[0], (0 if breaks is None else breaks.shape[0] - 1)
    q2 = np.empty((2, G, n_probs))
    order2 = np.empty((G, n_probs, 2))
    q2.view(np.uint64)[...] = NA_REAL_BITS
    order2.view(np.uint64)[...] = NA_REAL_BITS
    n_valid, n_na = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    hist, outside = np.zeros((G, n_bins), dtype=np.int64), np.zeros((G, 2), dtype=np.int64)
    for g, mask in enumerate(masks):
        have = mask & ~np.isnan(tri_raw)
        n_valid[g] = have.sum()
        n_na[g] = mask.sum() - have.sum()
        x, xc = tri_raw[have], tri_cor[have]
        if n_bins:
            hist[g] = np.histogram(x, bins=breaks)[0]
            outside[g, 0] = np.sum(x < breaks[0])
            outside[g, 1] = np.sum(x > breaks[-1])
        v = int(n_valid[g])
        if v == 0:
            continue
        order = np.argsort(x, kind="stable")
        xs, cs = x[order], xc[order]
        for k in range(n_probs):
            index = 1.0 + float(v - 1) * float(probs[k])
            lo, hi = int(math.floor(index)), int(math.ceil(index))
            order2[g, k, 0], order2[g, k, 1] = xs[lo - 1], xs[hi - 1]
            q2[1, g, k] = type7(xs[lo - 1], xs[hi - 1], index, float(lo))
            q2[0, g, k] = type7(cs[lo - 1], cs[hi - 1], index, float(lo))
    return q2, order2, n_valid, n_na, hist, outside
