"""Brute-force statement of icikt_class_matrix_f64's contract, from five full S x S matrices (cor, raw, pvalue, taumax,
completeness) over ALL pairs and a class index per sample.  Used by the CPU tests of the front end and the GPU tests of
the kernels; written without api._class_matrix_numpy: a plain loop over the cells, Python's sorted and the median rule.

Partners of cell (s, c): the samples t != s with cls[t] == c whose raw with s is not NA; n_valid[s, c] counts them.
med_raw[s, c]: R's median(raw, na.rm = TRUE) over the partners -- sorted ascending (a zero counts as +0), the value at
position (v - 1) >> 1, or mean() of it and the next when v is even.  med_cor[s, c]: the same rule on the cor cells that
belong to those one or two middle raw values.  No partner: NA_real_ in both."""
import math

import numpy as np

from tests.medians_checker import NA_REAL_BITS, bits, r_mean2   # noqa: F401  (bits, NA_REAL_BITS: for the tests)


def brute_class_matrix(out5, cls, n_class):
    """(med2 [2, S, n_class]: cor, raw; n_valid [S, n_class]); cls None: one class"""
    cor = np.asarray(out5[0], dtype=np.float64)
    raw = np.asarray(out5[1], dtype=np.float64)
    S = raw.shape[0]
    cls = [0] * S if cls is None else [int(k) for k in cls]
    med2 = np.empty((2, S, n_class), dtype=np.float64)
    med2.view(np.uint64)[...] = NA_REAL_BITS
    n_valid = np.zeros((S, n_class), dtype=np.int32)
    members = [[t for t in range(S) if cls[t] == c] for c in range(n_class)]
    for s in range(S):
        raw_s, cor_s = raw[s].tolist(), cor[s].tolist()
        for c in range(n_class):
            cells = [(raw_s[t] + 0.0, cor_s[t] + 0.0) for t in members[c]                   # (+ 0.0: a zero as +0)
                     if t != s and not math.isnan(raw_s[t])]
            v = len(cells)
            n_valid[s, c] = v
            if v == 0:
                continue
            cells = sorted(cells, key=lambda cell: cell[0])          # by raw; -0.0 == +0.0, and the sort is stable
            lo, hi = cells[(v - 1) >> 1], cells[v >> 1]
            med2[1, s, c] = lo[0] if v & 1 else r_mean2(lo[0], hi[0])
            med2[0, s, c] = lo[1] if v & 1 else r_mean2(lo[1], hi[1])
    return med2, n_valid


def interleaved(S=130):
    """classes of 1, 2, 3, 60 and 64 samples in shuffled order; class index 2 of the 6 stays empty
    (tests/test_gpu_medians._interleaved's layout)"""
    cls = np.repeat([0, 1, 3, 4, 5], [1, 2, 3, 60, 64]).astype(np.int32)
    assert cls.shape[0] == S
    np.random.default_rng(4).shuffle(cls)
    return cls, 6


def signal_matrix():
    """(X [60, 130], labels, names): every class adds its own feature profile to its members' columns, so a sample
    correlates with its class well above the others and the best two cells of its row are far apart; 8 % of the
    cells are missing; column 17 is constant (every pair of it carries a warning and an NA)."""
    cls, _n_class = interleaved()
    S, n = cls.shape[0], 60
    rng = np.random.default_rng(31)
    profile = rng.standard_normal((n, 6))
    X = np.asfortranarray(profile[:, cls] + 0.6 * rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    X[:, 17] = 1.5
    return X, [f"batch{k}" for k in cls], [f"s{i}" for i in range(S)]


def clear_nearest(med_raw, n_valid, gap=1e-9):
    """bool [S]: the sample has at least two cells with a partner and its two largest med_raw among them differ by
    more than `gap` -- where nearest_class does not hang on the last bits of a pair's value"""
    med_raw = np.asarray(med_raw, dtype=np.float64)
    clear = np.zeros(med_raw.shape[0], dtype=bool)
    for s in range(med_raw.shape[0]):
        have = sorted((float(v) for v, k in zip(med_raw[s], n_valid[s]) if k > 0), reverse=True)
        clear[s] = len(have) >= 2 and have[0] - have[1] > gap
    return clear
