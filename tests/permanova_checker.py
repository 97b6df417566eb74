"""Brute-force checker of icikt_permanova_f64 and its front end, in plain loops, Python ints and
Fractions.  Nothing of it comes from the library or from icikendalltau_amd.api.

The rule.  A pair i < j is a value iff its raw is not NaN.  A value's squared dissimilarity is the integer q: with
d = 1.0 - raw and e = d * d as doubles (-0 taken as +0), q is the exact rational e 2^50 rounded to the nearest integer,
halves to the even one.  Q is the sum of q over all pairs; A_c of a labelling the sum over the pairs whose two samples
both have class c.  With n_c the labelling's class sizes and C' the classes that have a sample,
SS_T = Q / (S 2^50), SS_W = sum_c A_c / (n_c 2^50), SS_A = SS_T - SS_W, F = (SS_A / (C' - 1)) / (SS_W / (S - C')),
R2 = SS_A / SS_T.  F is undefined when C' < 2, S <= C' or SS_T = 0, and +Inf when SS_W = 0 < SS_A.  With an NA pair
nothing is summed per class and every statistic is NA.
"""
import math
from fractions import Fraction

import numpy as np

from tests.anosim_checker import bits, documented_permutations, na_real   # noqa: F401  (shared helpers, re-exported)

SCALE = 2 ** 50


def quantise(raw):
    """q of one raw value that is not NaN: Fraction arithmetic behind the two double operations"""
    raw = float(raw) + 0.0
    d = 1.0 - raw
    e = d * d
    return round(Fraction(e) * SCALE)          # (round() of a Fraction: halves go to the even integer)


def to_double(x):
    if x is None:
        return na_real()
    return float(x)                             # (Fraction -> float: correctly rounded; inf stays inf)


def statistic(S, Q, A, sizes):
    """(F, R2, SS_T, SS_W, SS_A, df_among, df_within): Fractions and ints; F None when undefined, math.inf when
    SS_W = 0 < SS_A; R2 None when SS_T = 0"""
    used = [c for c in range(len(sizes)) if sizes[c] > 0]
    ss_t = Fraction(Q, S * SCALE)
    ss_w = sum((Fraction(A[c], sizes[c] * SCALE) for c in used), Fraction(0))
    ss_a = ss_t - ss_w
    df_a, df_w = len(used) - 1, S - len(used)
    if len(used) < 2 or df_w <= 0 or ss_t == 0:
        F = None
    elif ss_w == 0:
        F = math.inf
    else:
        F = (ss_a / df_a) / (ss_w / df_w)
    return F, (ss_a / ss_t if ss_t != 0 else None), ss_t, ss_w, ss_a, df_a, df_w


def brute_permanova(raw, cls, n_class, perms):
    """A dict of everything icikt_permanova_f64 and the front end return, from `raw` [S, S], the observed class codes
    [S], n_class and the labellings to compare with [n_perm, S]."""
    raw = np.asarray(raw, dtype=np.float64)
    cls = [int(v) for v in cls]
    S = len(cls)
    perms = np.asarray(perms, dtype=np.int64).reshape(-1, S)
    labs = [cls] + [[int(v) for v in row] for row in perms]
    pairs, n_na, Q = [], 0, 0
    for i in range(S):
        for j in range(i + 1, S):
            v = float(raw[i, j])
            if v != v:
                n_na += 1
                continue
            q = quantise(v)
            assert 0 <= q <= 2 ** 52
            pairs.append((i, j, q))
            Q += q
    class_q, sizes = [], []
    for lab in labs:
        A, size = [0] * n_class, [0] * n_class
        for c in lab:
            size[c] += 1
        if n_na == 0:
            for i, j, q in pairs:
                if lab[i] == lab[j]:
                    A[lab[i]] += q
        class_q.append(A)
        sizes.append(size)
    n_perm = len(labs) - 1
    if n_na == 0:
        stats = [statistic(S, Q, A, size) for A, size in zip(class_q, sizes)]
    else:
        used = sum(1 for n in sizes[0] if n > 0)
        stats = [(None, None, None, None, None, used - 1, S - used)] * (1 + n_perm)
    obs, Fs = stats[0], [s[0] for s in stats[1:]]
    n_undefined = sum(1 for f in Fs if f is None)
    n_ge = 0 if obs[0] is None else sum(1 for f in Fs if f is not None and f >= obs[0])
    return {
        "n_pairs": np.array([len(pairs), n_na], dtype=np.int64), "q_total": Q, "class_q": class_q, "sizes": sizes,
        "n_ge": n_ge, "n_undefined": n_undefined,
        "statistic": to_double(obs[0]), "r2": to_double(obs[1]),
        "pvalue": na_real() if obs[0] is None else float(Fraction(1 + n_ge, 1 + n_perm)),
        "ss_total": to_double(obs[2]), "ss_within": to_double(obs[3]), "ss_among": to_double(obs[4]),
        "df_among": obs[5], "df_within": obs[6],
        "perm_statistic": np.array([to_double(f) for f in Fs], dtype=np.float64),
        "class_size": np.array(sizes[0], dtype=np.int64),
        "class_ss": np.array([to_double(Fraction(a, n * SCALE) if (n and n_na == 0) else None)
                              for a, n in zip(class_q[0], sizes[0])], dtype=np.float64),
        "exact": (obs, Fs),
    }
