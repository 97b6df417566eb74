"""Brute-force statement of icikt_class_medians_f64's contract, from five full S x S matrices (cor, raw, pvalue, taumax,
completeness) and a class index per sample.  Used by the CPU tests of the front end and the GPU tests of the kernels.

Partners of sample s: the other samples of its class whose raw with s is not NA; n_valid[s] counts them.
med_raw[s]: R's median(raw, na.rm = TRUE) over the partners -- sort ascending (a zero counts as +0), the middle value, or
mean() of the two middle values.  med_cor[s]: the same rule on the cor cells that belong to those one or two middle raw
values (cor is a monotone map of raw, so these ARE the middle cor values).  No partner: NA_real_ in both."""
import math

import numpy as np

NA_REAL_BITS = np.uint64(0x7FF00000000007A2)
R_NAN_BITS = np.uint64(0x7FF8000000000000)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _from_bits(b):
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def r_mean2(a, b):
    """R's mean(c(a, b)) (long double accumulation: the correctly rounded midpoint), a zero as +0."""
    s = a + b
    if math.isfinite(s):
        return 0.5 * s + 0.0
    if math.isfinite(a) and math.isfinite(b):
        return 0.5 * a + 0.5 * b + 0.0
    return _from_bits(R_NAN_BITS) if math.isnan(s) else s


def class_pairs(cls, n_class=None):
    """(pi, pj) of the within-class pairs in the call's order: class by class, combn order over a class's members."""
    cls = np.asarray(cls)
    n_class = int(cls.max()) + 1 if n_class is None else n_class
    pi, pj = [], []
    for k in range(n_class):
        members = np.nonzero(cls == k)[0]
        x, y = np.triu_indices(len(members), k=1)      # row-major upper triangle == combn order
        pi.append(members[x])
        pj.append(members[y])
    if not pi:
        return np.empty(0, dtype=np.int32), np.empty(0, dtype=np.int32)
    return np.concatenate(pi).astype(np.int32), np.concatenate(pj).astype(np.int32)


def brute_medians(out5, cls):
    """(med2 [2, S]: cor, raw; n_valid [S])"""
    cor = np.ascontiguousarray(out5[0], dtype=np.float64)
    raw = np.ascontiguousarray(out5[1], dtype=np.float64)
    S = raw.shape[0]
    cls = np.zeros(S, dtype=np.int64) if cls is None else np.asarray(cls)
    med2 = np.empty((2, S), dtype=np.float64)
    med2.view(np.uint64)[...] = NA_REAL_BITS
    n_valid = np.zeros(S, dtype=np.int32)
    for s in range(S):
        ok = (cls == cls[s]) & ~np.isnan(raw[s])
        ok[s] = False
        partners = np.nonzero(ok)[0]
        v = len(partners)
        n_valid[s] = v
        if v == 0:
            continue
        # ascending by raw with -0.0 == +0.0 (the sort compares the doubles, and is stable)
        order = np.argsort(raw[s, partners], kind="stable")
        lo, hi = partners[order[(v - 1) // 2]], partners[order[v // 2]]
        for q, mat in ((0, cor), (1, raw)):
            a, b = float(mat[s, lo]) + 0.0, float(mat[s, hi]) + 0.0     # (+ 0.0: a zero as +0)
            med2[q, s] = a if v % 2 else r_mean2(a, b)
    return med2, n_valid
