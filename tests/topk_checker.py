"""Brute-force checker of the top-k selection (icikt_topk_f64 / api.ici_kendalltau_topk): from five full S x S
matrices, per column, plain Python sorting of (-key, partner) tuples, the key taken from the bits of `raw` as the
library's dbl_sortable takes it (so -0.0 sorts below +0.0).  Independent of the package's own selector."""
import numpy as np

NA_REAL_BITS = 0x7FF00000000007A2   # R's NA_real_
_M64 = (1 << 64) - 1


def sortable_key(bits: int) -> int:
    """Monotone in the double whose bits these are; NaN never gets here."""
    return (~bits & _M64) if bits >> 63 else (bits | (1 << 63))


def ranked_partners(raw):
    """Per column c the partners j != c whose raw[c, j] is not NaN, best first: raw descending by the bits, ties by
    the smaller index."""
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    S = raw.shape[0]
    bits = raw.view(np.uint64).tolist()
    nan = np.isnan(raw).tolist()
    out = []
    for c in range(S):
        row, bad = bits[c], nan[c]
        cand = [(-sortable_key(row[j]), j) for j in range(S) if j != c and not bad[j]]
        cand.sort()
        out.append([j for _key, j in cand])
    return out


def brute_topk(mats5, k, ranked=None):
    """(idx [S, k] int32, -1 padded; vals5 [5, S, k], NA_real_ padded; n_valid [S]) from the five matrices
    (cor, raw, pvalue, taumax, completeness).  ranked: ranked_partners(raw) when the caller has it already."""
    mats5 = [np.ascontiguousarray(m, dtype=np.float64) for m in mats5]
    S = mats5[1].shape[0]
    if ranked is None:
        ranked = ranked_partners(mats5[1])
    idx = np.full((S, k), -1, dtype=np.int32)
    vals = np.empty((5, S, k), dtype=np.uint64)
    vals[...] = NA_REAL_BITS
    n_valid = np.zeros(S, dtype=np.int32)
    views = [m.view(np.uint64) for m in mats5]
    for c in range(S):
        sel = ranked[c][:k]
        n_valid[c] = len(sel)
        idx[c, :len(sel)] = sel
        for q in range(5):
            vals[q, c, :len(sel)] = views[q][c, sel]
    return idx, vals.view(np.float64), n_valid
