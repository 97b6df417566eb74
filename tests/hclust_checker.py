"""Brute-force reference for icikt_hclust_f64 (plain numpy and Python floats, no GPU): the rule as a naive O(S^3) loop
over a full S x S matrix of raw.

The rule.  The similarity of two samples is the pair's raw, -0 equal to +0; NaN: none.  A cluster lives in the slot of
its smallest sample.  Each step merges the best live pair of clusters a < b into a, in the strict order: the larger
similarity first, then the smaller a, then the smaller b.  The merged cluster's similarity to a live cluster k is NaN if
either old one is; else the smaller (complete), the larger (single), or (n_a * w_a + n_b * w_b) / (n_a + n_b) in Python
floats -- two products, two sums, one division, each rounded once (average).  Merging ends at the first step whose best
similarity is NaN or, with min_raw, not >= min_raw.  Components are numbered by their smallest sample."""
import numpy as np

from tests.mst_checker import bits, sort_key

METHODS = ("complete", "average", "single")


def _key_matrix(V):
    """the order-preserving uint64 keys of the library's kernels; 0 (which no double maps to) where V is NaN"""
    K = np.zeros(V.shape, dtype=np.uint64)
    ok = ~np.isnan(V)
    K[ok] = sort_key(V[ok])
    return K


def average_update(na, wa, nb, wb):
    """the rule's average: two products, two sums, one division in Python floats, each rounded once"""
    return (na * wa + nb * wb) / (na + nb)


def brute_hclust(raw_matrix, method, min_raw=None, average=average_update):
    """(ma, mb, msize int32 [n_merges]; mraw float64 [n_merges]; component int32 [S]; n_components).  `average`: the
    update of average linkage; another one only for a test that shows a design can tell the two apart."""
    assert method in METHODS
    with np.errstate(invalid="ignore"):
        V = np.array(raw_matrix, dtype=np.float64) + 0.0        # (+ 0.0: -0 becomes +0)
    S = V.shape[0]
    V[np.tril_indices(S)] = np.nan
    V = np.fmax(V, V.T)                                         # the upper triangle, mirrored; the diagonal stays NaN
    K = _key_matrix(V)
    alive = [True] * S
    size = [1] * S
    slot = list(range(S))
    ma, mb, msize, mraw = [], [], [], []
    for _step in range(S - 1):
        T = np.triu(K, k=1)                                     # (rows and columns of dead slots are zeroed below)
        flat = int(np.argmax(T))                                # the first maximum in row-major order: smaller a, then b
        a, b = divmod(flat, S)
        if T[a, b] == 0:
            break
        best = float(V[a, b])
        if min_raw is not None and not np.isnan(min_raw) and not best >= min_raw:
            break
        assert a < b and alive[a] and alive[b]
        na, nb = float(size[a]), float(size[b])
        for k in range(S):
            if k == a or k == b or not alive[k]:
                continue
            wa, wb = float(V[a, k]), float(V[b, k])
            if wa != wa or wb != wb:
                w = float("nan")
            elif method == "complete":
                w = min(wa, wb)
            elif method == "single":
                w = max(wa, wb)
            else:
                w = average(na, wa, nb, wb) + 0.0
            V[a, k] = V[k, a] = w
        V[b, :] = V[:, b] = np.nan                              # slot b is no cluster any more
        K[b, :] = K[:, b] = 0
        K[a, :] = _key_matrix(V[a, :])
        K[:, a] = K[a, :]
        alive[b] = False
        size[a] += size[b]
        slot[b] = a
        ma.append(a)
        mb.append(b)
        msize.append(size[a])
        mraw.append(best)
    component = np.empty(S, dtype=np.int32)
    n_comp = 0
    for s in range(S):                                          # a slot merges into a smaller one: one ascending pass
        if slot[s] == s:
            component[s] = n_comp
            n_comp += 1
        else:
            component[s] = component[slot[s]]
    return (np.asarray(ma, dtype=np.int32), np.asarray(mb, dtype=np.int32), np.asarray(msize, dtype=np.int32),
            np.asarray(mraw, dtype=np.float64), component, n_comp)


def members(ma, mb, S):
    """per merge, the frozenset of samples of the new cluster"""
    sets = [frozenset([s]) for s in range(S)]
    out = []
    for a, b in zip(np.asarray(ma).tolist(), np.asarray(mb).tolist()):
        sets[a] = sets[a] | sets[b]
        out.append(sets[a])
    return out


__all__ = ["METHODS", "bits", "brute_hclust", "members"]
