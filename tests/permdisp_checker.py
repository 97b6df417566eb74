"""Brute-force checker of icikt_permdisp_f64 and its front end, in plain loops, Python ints,
Fractions and 120-digit decimals.  Nothing of it comes from the library or from icikendalltau_amd.api.

The rule.  A pair i < j is a value iff its raw is not NaN; its q is PERMANOVA's (tests/permanova_checker.quantise), a
pair that is no value adds 0.  T[i][c] is the sum of q_ij over the samples j != i of class c.  With n_c the class sizes
and A_c the sum of q over the pairs inside class c, X[i][c] = n_c T[i][c] - A_c and the squared distance of sample i to
the centroid of class c is X / (n_c^2 2^50); the distance z is the double nearest to sqrt(|X|) / (n_c 2^25).  The
statistic is the one-way ANOVA F of the own-class distances, as fractions; the permutation test permutes the residuals
z_i - m_c (m_c the double nearest to the class mean, one IEEE subtraction).  With an NA pair every statistic, distance
and centroid cell is NA; the table stays as summed.
"""
import decimal
import math
from fractions import Fraction

import numpy as np

from tests.anosim_checker import bits, documented_permutations, na_real   # noqa: F401  (shared helpers, re-exported)
from tests.permanova_checker import quantise, to_double

_CTX = decimal.Context(prec=120)


def na_array(shape):
    a = np.empty(shape, dtype=np.float64)
    a.view(np.uint64)[...] = bits(na_real())[0]
    return a


def _nearest_double(x):
    """the double nearest to the positive 120-digit decimal x: its conversion and that value's two neighbours compared"""
    f = float(x)
    best, err = None, None
    for cand in (math.nextafter(f, 0.0), f, math.nextafter(f, math.inf)):
        e = abs(_CTX.subtract(decimal.Decimal(cand), x))
        if err is None or e < err:
            best, err = cand, e
    return best


def distance(X, n):
    """the double nearest to sqrt(|X|) / (n 2^25), through a 120-digit square root"""
    X = abs(int(X))
    if X == 0:
        return 0.0
    return _nearest_double(_CTX.divide(_CTX.sqrt(decimal.Decimal(X)), decimal.Decimal(n * 2 ** 25)))


def anova(values, lab, n_class):
    """(F, SS_A, SS_W, df_among, df_within) of the one-way ANOVA of `values` (anything Fraction() takes exactly) over the
    labels `lab`, from the class means: F None when C' < 2, S <= C' or all values are equal; inf when SS_W = 0 < SS_A"""
    v = [Fraction(x) for x in values]
    S = len(v)
    groups = [[v[i] for i in range(S) if lab[i] == c] for c in range(n_class)]
    groups = [g for g in groups if g]
    grand = sum(v, Fraction(0)) / S
    ss_a = sum((len(g) * (sum(g, Fraction(0)) / len(g) - grand) ** 2 for g in groups), Fraction(0))
    ss_w = Fraction(0)
    for g in groups:
        mean = sum(g, Fraction(0)) / len(g)
        ss_w += sum(((x - mean) ** 2 for x in g), Fraction(0))
    df_a, df_w = len(groups) - 1, S - len(groups)
    if df_a < 1 or df_w <= 0 or all(x == v[0] for x in v):
        F = None
    elif ss_w == 0:
        F = math.inf
    else:
        F = (ss_a / df_a) / (ss_w / df_w)
    return F, ss_a, ss_w, df_a, df_w


def brute_table(raw, cls, n_class):
    """(n_values, n_na, Q, T [S][n_class], A [n_class], sizes [n_class]) in plain loops over all ordered pairs"""
    raw = np.asarray(raw, dtype=np.float64)
    cls = [int(v) for v in cls]
    S = len(cls)
    q = {}
    n_na, Q = 0, 0
    A, sizes = [0] * n_class, [0] * n_class
    for c in cls:
        sizes[c] += 1
    for i in range(S):
        for j in range(i + 1, S):
            v = float(raw[i, j])
            if v != v:
                n_na += 1
                q[(i, j)] = 0
                continue
            q[(i, j)] = quantise(v)
            Q += q[(i, j)]
            if cls[i] == cls[j]:
                A[cls[i]] += q[(i, j)]
    T = [[0] * n_class for _ in range(S)]
    for i in range(S):
        for j in range(S):
            if j != i:
                T[i][cls[j]] += q[(min(i, j), max(i, j))]
    return S * (S - 1) // 2 - n_na, n_na, Q, T, A, sizes


def brute_permdisp(raw, cls, n_class, perms):
    """A dict of everything icikt_permdisp_f64 and the front end return, from `raw` [S, S], the observed class codes [S],
    n_class and the labellings to compare with [n_perm, S]."""
    return permdisp_tail(brute_table(raw, cls, n_class), cls, n_class, perms)


def permdisp_tail(table, cls, n_class, perms):
    """brute_permdisp from its table on: `table` is brute_table's tuple (n_values, n_na, Q, T [S][n_class], A [n_class],
    sizes [n_class]) in Python ints, from whatever summed it (tests/designed_tau.permdisp_table sums it from a design's
    integers); everything behind it -- the distances, the ANOVA and the permutation test -- is this function's."""
    cls = [int(v) for v in cls]
    S = len(cls)
    perms = [[int(v) for v in row] for row in np.asarray(perms, dtype=np.int64).reshape(-1, S)]
    n_val, n_na, Q, T, A, sizes = table
    for c in range(n_class):
        assert 2 * A[c] == sum(T[i][c] for i in range(S) if cls[i] == c)
    used = [c for c in range(n_class) if sizes[c] > 0]
    n_perm = len(perms)
    NA = na_real()
    zc = na_array((S, n_class))
    out = {"n_pairs": np.array([n_val, n_na], dtype=np.int64), "q_total": Q, "t": T, "class_q": A,
           "class_size": np.array(sizes, dtype=np.int64), "df_among": len(used) - 1, "df_within": S - len(used)}
    if n_na > 0:
        out.update(distances=na_array(S), centroid_distance=zc, class_mean_distance=na_array(n_class),
                   nearest_centroid=np.full(S, -1, dtype=np.int32), n_negative=0, statistic=NA, pvalue=NA, ss_among=NA,
                   ss_within=NA, n_ge=0, n_undefined=n_perm, perm_statistic=na_array(n_perm),
                   exact=((None, None, None, len(used) - 1, S - len(used)), [None] * n_perm), x=None)
        return out
    X = [[sizes[c] * T[i][c] - A[c] if sizes[c] else 0 for c in range(n_class)] for i in range(S)]
    for i in range(S):
        for c in used:
            assert abs(X[i][c]) < 2 ** 84
            zc[i, c] = distance(X[i][c], sizes[c])
    z = [float(zc[i, cls[i]]) for i in range(S)]
    nearest = []
    for i in range(S):
        best = used[0]
        for c in used[1:]:
            if Fraction(abs(X[i][c]), sizes[c] ** 2) < Fraction(abs(X[i][best]), sizes[best] ** 2):
                best = c
        nearest.append(best)
    means = na_array(n_class)
    for c in used:
        means[c] = float(sum((Fraction(z[i]) for i in range(S) if cls[i] == c), Fraction(0)) / sizes[c])
    obs = anova(z, cls, n_class)
    resid = [z[i] - float(means[cls[i]]) for i in range(S)]
    Fs = [anova(resid, lab, n_class)[0] for lab in perms]
    n_undefined = sum(1 for f in Fs if f is None)
    n_ge = 0 if obs[0] is None else sum(1 for f in Fs if f is not None and f >= obs[0])
    out.update(distances=np.array(z, dtype=np.float64), centroid_distance=zc, class_mean_distance=means,
               nearest_centroid=np.array(nearest, dtype=np.int32),
               n_negative=sum(1 for i in range(S) if X[i][cls[i]] < 0),
               statistic=to_double(obs[0]), pvalue=NA if obs[0] is None else float(Fraction(1 + n_ge, 1 + n_perm)),
               ss_among=to_double(obs[1]), ss_within=to_double(obs[2]), n_ge=n_ge, n_undefined=n_undefined,
               perm_statistic=np.array([to_double(f) for f in Fs], dtype=np.float64), exact=(obs, Fs), x=X, residuals=resid)
    return out
