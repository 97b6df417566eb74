"""Brute-force checker of the threshold selection (icikt_edges_f64 / api.ici_kendalltau_edges): from five full S x S
matrices (cor, raw, pvalue, taumax, completeness) the upper-triangle pairs in combn order that pass the rule, by
numpy's own comparisons on out5[1], out5[2] and out5[4].  Independent of the package's own selector."""
import numpy as np


def combn_pairs(S):
    """(i, j) of combn(S, 2): i ascending, then j ascending."""
    i = np.repeat(np.arange(S), np.arange(S - 1, -1, -1))
    j = np.concatenate([np.arange(a + 1, S) for a in range(S)]) if S > 1 else np.empty(0, dtype=np.int64)
    return i.astype(np.int32), j.astype(np.int32)


def brute_edges(mats5, min_raw=None, max_pvalue=None, min_completeness=None, absolute=False):
    """(ei, ej int32; vals5 [5, m]; n_edges; degree [S] int64): ALL matching pairs.  A bound of None is no bound."""
    mats5 = [np.ascontiguousarray(m, dtype=np.float64) for m in mats5]
    S = mats5[1].shape[0]
    pi, pj = combn_pairs(S)
    raw, pvalue, comp = mats5[1][pi, pj], mats5[2][pi, pj], mats5[4][pi, pj]
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(raw)
        if min_raw is not None:
            ok = ok & ((np.abs(raw) if absolute else raw) >= min_raw)
        if max_pvalue is not None:
            ok = ok & (pvalue <= max_pvalue)
        if min_completeness is not None:
            ok = ok & (comp >= min_completeness)
    ei, ej = pi[ok], pj[ok]
    vals = np.empty((5, ei.shape[0]), dtype=np.float64)
    for q in range(5):
        vals[q] = mats5[q][ei, ej]
    degree = np.zeros(S, dtype=np.int64)
    np.add.at(degree, ei, 1)
    np.add.at(degree, ej, 1)
    return ei, ej, vals, int(ei.shape[0]), degree


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same(got, ref, max_edges=None):
    """got: (ei, ej, vals5, n_edges, degree, ...) as Context.edges returns it; ref: brute_edges' tuple.  With max_edges
    the lists are the first max_edges of the reference's; n_edges and degree are the full counts either way.  The
    values are compared BITWISE."""
    ei, ej, vals, n_edges, degree = got[:5]
    rei, rej, rvals, rn, rdeg = ref
    m = rn if max_edges is None else min(rn, max_edges)
    assert n_edges == rn, (n_edges, rn)
    assert np.array_equal(degree, rdeg)
    assert ei.shape == (m,) and ej.shape == (m,) and vals.shape == (5, m)
    assert np.array_equal(ei, rei[:m])
    assert np.array_equal(ej, rej[:m])
    assert np.array_equal(bits(vals), bits(rvals[:, :m]))
