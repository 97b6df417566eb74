"""Brute-force statement of the class tables of icikt_ref_cross_f64 / api.ici_kendalltau_cross(reference_classes=...),
from the rectangle's five Sq x Sr matrices (cor, raw, pvalue, taumax, completeness) and a class index per REFERENCE
column.  Used by the CPU tests of the front end and the GPU tests of the kernel; written without the api helpers: a plain
loop over the cells, Python's sorted and the median rule.

Partners of cell (q, c): the reference columns r with ref_cls[r] == c whose raw with q is not NA -- a column that occurs
in both matrices is a partner like any other, there is no own sample on a rectangle; n_valid[q, c] counts them.
med_raw[q, c]: R's median(raw, na.rm = TRUE) over the partners -- sorted ascending (a zero counts as +0), the value at
position (v - 1) >> 1, or mean() of it and the next when v is even.  med_cor[q, c]: the same rule on the cor cells that
belong to those one or two middle raw values.  No partner: NA_real_ in both."""
import math

import numpy as np

from tests.medians_checker import NA_REAL_BITS, bits, r_mean2   # noqa: F401  (bits, NA_REAL_BITS: for the tests)


def brute_cross_class(rect5, ref_cls, n_class):
    """(med2 [2, Sq, n_class]: cor, raw; n_valid [Sq, n_class])"""
    cor = np.asarray(rect5[0], dtype=np.float64)
    raw = np.asarray(rect5[1], dtype=np.float64)
    Sq, Sr = raw.shape
    ref_cls = [int(k) for k in ref_cls]
    assert len(ref_cls) == Sr
    med2 = np.empty((2, Sq, n_class), dtype=np.float64)
    med2.view(np.uint64)[...] = NA_REAL_BITS
    n_valid = np.zeros((Sq, n_class), dtype=np.int32)
    members = [[r for r in range(Sr) if ref_cls[r] == c] for c in range(n_class)]
    for q in range(Sq):
        raw_q, cor_q = raw[q].tolist(), cor[q].tolist()
        for c in range(n_class):
            cells = [(raw_q[r] + 0.0, cor_q[r] + 0.0) for r in members[c] if not math.isnan(raw_q[r])]   # (+ 0.0: a zero as +0)
            v = len(cells)
            n_valid[q, c] = v
            if v == 0:
                continue
            cells = sorted(cells, key=lambda cell: cell[0])          # by raw; -0.0 == +0.0, and the sort is stable
            lo, hi = cells[(v - 1) >> 1], cells[v >> 1]
            med2[1, q, c] = lo[0] if v & 1 else r_mean2(lo[0], hi[0])
            med2[0, q, c] = lo[1] if v & 1 else r_mean2(lo[1], hi[1])
    return med2, n_valid


def nearest(med_raw, n_valid, levels):
    """per query the level of the first largest med_raw among the cells with a partner, None without one"""
    out = []
    for row, cnt in zip(np.asarray(med_raw, dtype=np.float64).tolist(), np.asarray(n_valid).tolist()):
        best = None
        for c, (v, k) in enumerate(zip(row, cnt)):
            if k > 0 and (best is None or v > row[best]):
                best = c
        out.append(None if best is None else levels[best])
    return out
