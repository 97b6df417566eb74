"""Brute-force checker of icikt_pcoa_f64 and its front end, in plain loops, Python ints and
floats.  Nothing of it comes from the library or from icikendalltau_amd.api.

The rule.
 1. A pair's raw is the double of its kept key, -0 taken as +0.  A pair whose raw is NaN makes the whole result NA;
    n_na counts them, and the integers below are still summed (an NA pair adds 0).
 2. q_ij = PERMANOVA's integer (tests/permanova_checker.quantise: (1 - raw)^2 in two double operations, times 2^50,
    rounded half to even) and e^_ij = q_ij 2^-50, exact in a double because q <= 2^52; e^_ii = 0.
 3. R_i = sum_j q_ij and T = sum_i R_i = 2 Q are integers.
 4. m_i = R_i / (S 2^50) and m-bar = T / (S^2 2^50): each Python's int / int, one correctly rounded conversion.
 5. G_ij = -0.5 * ((e^_ij - (m_i + m_j)) + m-bar): four double operations in this order (a Python float operation is
    one IEEE operation, nothing is contracted).  G is symmetric to the bit.
 6. total_inertia = Q / (S 2^50), the trace of G in exact arithmetic, correctly rounded.
 7. The result is the k algebraically largest eigenvalues of G, descending, with orthonormal eigenvectors;
    coordinates[:, a] = vectors[:, a] sqrt(lambda_a) where lambda_a > 0, else 0; n_positive counts the positive ones;
    proportion = lambda / total_inertia.  Sign: a vector's component of largest magnitude is positive, the smallest
    index deciding among equal magnitudes.
"""
from fractions import Fraction

import numpy as np

from tests.anosim_checker import bits, na_real   # noqa: F401  (shared helpers, re-exported)
from tests.permanova_checker import SCALE, quantise


def brute_gower(raw):
    """(n_values, n_na, Q, R [S] of Python ints, G [S, S] float64 or None with an NA pair) in plain loops"""
    raw = np.asarray(raw, dtype=np.float64)
    S = raw.shape[0]
    q = [[0] * S for _ in range(S)]
    n_na = 0
    for i in range(S):
        for j in range(i + 1, S):
            v = float(raw[i, j])
            if v != v:
                n_na += 1
                continue
            q[i][j] = q[j][i] = quantise(v)
            assert 0 <= q[i][j] <= 2 ** 52
    R = [sum(row) for row in q]
    T = sum(R)
    assert T % 2 == 0
    n_val = S * (S - 1) // 2 - n_na
    if n_na > 0:
        return n_val, n_na, T // 2, R, None
    m = [R[i] / (S * SCALE) for i in range(S)]
    grand = T / (S * S * SCALE)
    G = np.empty((S, S), dtype=np.float64)
    for i in range(S):
        for j in range(S):
            e = q[i][j] * 2.0 ** -50                   # (exact: q <= 2^52)
            G[i, j] = -0.5 * ((e - (m[i] + m[j])) + grand)
    return n_val, n_na, T // 2, R, G


def total_inertia(Q, S):
    return float(Fraction(Q, S * SCALE))


def largest(G, k):
    """(the k largest eigenvalues of G, descending; all eigenvalues, ascending) by numpy.linalg.eigh"""
    w = np.linalg.eigh(G)[0]
    return w[::-1][:k].copy(), w


def sign_rule_holds(vectors):
    """every column's component of largest magnitude -- the first of equal magnitudes -- is positive"""
    V = np.asarray(vectors, dtype=np.float64)
    for a in range(V.shape[1]):
        col = V[:, a]
        best = 0
        for i in range(1, col.size):
            if abs(col[i]) > abs(col[best]):
                best = i
        if not col[best] > 0:
            return False
    return True


def coordinates(vectors, lam):
    V = np.asarray(vectors, dtype=np.float64)
    out = np.zeros_like(V)
    for a, l in enumerate(lam):
        if l > 0:
            out[:, a] = V[:, a] * np.sqrt(l)
    return out
