"""Brute-force checker of icikt_cross_f64 / api.ici_kendalltau_cross: the rectangle's pair list on the stacked matrix,
the [query, reference] block of a full result, and every query's top-k by plain Python sorting of (-key, reference
index) tuples, the key taken from the bits of `raw` as the library's sortable key takes it (so -0.0 sorts below +0.0).
Independent of the package's own selector; shared by tests/test_cross_host.py and tests/test_gpu_cross.py."""
import numpy as np

from tests.topk_checker import NA_REAL_BITS, sortable_key

KEYS = ("cor", "raw", "pvalue", "taumax", "completeness")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rect_pairs(Sq, Sr):
    """The rectangle on the stacked matrix [query, reference], query-major: pair p = q * Sr + r is (q, Sq + r)."""
    pi = np.repeat(np.arange(Sq, dtype=np.int32), Sr)
    pj = (Sq + np.tile(np.arange(Sr, dtype=np.int32), Sq)).astype(np.int32)
    return pi, pj


def rect_block(mats5, Sq):
    """[5, Sq, Sr]: rows the query columns, columns the reference columns, of five matrices of the stacked matrix."""
    return np.stack([np.ascontiguousarray(np.asarray(m, dtype=np.float64)[:Sq, Sq:]) for m in mats5])


def brute_cross_topk(rect5, k):
    """(idx [Sq, k] int32, -1 padded; vals5 [5, Sq, k], NA_real_ padded; n_valid [Sq]) from the rectangle's five
    matrices (cor, raw, pvalue, taumax, completeness)."""
    rect5 = [np.ascontiguousarray(m, dtype=np.float64) for m in rect5]
    Sq, Sr = rect5[1].shape
    raw_bits = rect5[1].view(np.uint64).tolist()
    nan = np.isnan(rect5[1]).tolist()
    views = [m.view(np.uint64) for m in rect5]
    idx = np.full((Sq, k), -1, dtype=np.int32)
    vals = np.empty((5, Sq, k), dtype=np.uint64)
    vals[...] = NA_REAL_BITS
    n_valid = np.zeros(Sq, dtype=np.int32)
    for q in range(Sq):
        cand = sorted((-sortable_key(raw_bits[q][r]), r) for r in range(Sr) if not nan[q][r])
        sel = [r for _key, r in cand[:k]]
        n_valid[q] = len(sel)
        idx[q, :len(sel)] = sel
        for f in range(5):
            vals[f, q, :len(sel)] = views[f][q, sel]
    return idx, vals.view(np.float64), n_valid


def max_taumax(rect5):
    """max(taumax, na.rm = TRUE) over the rectangle; -inf without a value (R's max(numeric(0)))."""
    t = np.asarray(rect5[3], dtype=np.float64).ravel()
    t = t[~np.isnan(t)]
    return float(t.max()) if t.size else -np.inf


def assert_topk_same(idx, vals, n_valid, ref):
    """Integers equal, doubles bitwise equal, the padding -1 / NA_real_ exactly behind n_valid entries."""
    ridx, rvals, rn = ref
    assert np.array_equal(n_valid, rn)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(bits(vals), bits(rvals))
    pad = idx < 0
    assert np.array_equal(pad, np.arange(idx.shape[1])[None, :] >= np.asarray(n_valid)[:, None])
    for f in range(5):
        assert np.all(bits(vals[f])[pad] == NA_REAL_BITS)
