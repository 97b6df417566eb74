"""Brute-force reference for icikt_mst_f64 (plain numpy, no GPU): the maximum spanning forest of the samples under raw
by Kruskal in the strict edge order, and a verifier that does not go through Kruskal.

The rule.  A pair i < j is a candidate edge iff raw[i, j] is not NaN and, with min_raw, raw[i, j] >= min_raw (a plain
comparison of doubles).  Strict edge order: the larger raw first, compared through the order-preserving 64-bit key of
the library's kernels (so -0 equals +0), equal keys by the smaller combn index (i ascending, then j ascending).  The
order is total, so the forest is unique."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sort_key(v):
    """colsort::cor_key of values that are not NaN, as uint64: order-preserving, -0 == +0"""
    b = bits(np.asarray(v, dtype=np.float64) + 0.0)          # (+ 0.0: -0 becomes +0)
    top = np.uint64(1) << np.uint64(63)
    return np.where(b >> np.uint64(63) != 0, ~b, b | top)


def candidates(raw_matrix, min_raw=None):
    """(ci, cj, key, idx) of the candidate edges in the STRICT ORDER; idx: the combn index"""
    raw_matrix = np.asarray(raw_matrix, dtype=np.float64)
    S = raw_matrix.shape[0]
    iu, ju = np.triu_indices(S, k=1)                          # row-major upper triangle == combn order
    raw = raw_matrix[iu, ju]
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(raw)
        if min_raw is not None and not np.isnan(min_raw):
            ok &= raw >= min_raw
    idx = np.flatnonzero(ok)
    key = sort_key(raw[idx])
    order = np.lexsort((idx, ~key))                           # ~key ascending: key descending
    idx = idx[order]
    return iu[idx], ju[idx], key[order], idx


def _labels(parent):
    """component labels 0, 1, ... in order of each component's smallest sample"""
    S = len(parent)
    label, out, n = {}, np.empty(S, dtype=np.int32), 0
    for s in range(S):
        r = s
        while parent[r] != r:
            r = parent[r]
        if r not in label:
            label[r] = n
            n += 1
        out[s] = label[r]
    return out, n


def brute_mst(raw_matrix, min_raw=None):
    """(ti, tj int32: the forest's edges in the strict order; component [S] int32; n_components)"""
    S = np.asarray(raw_matrix).shape[0]
    ci, cj, _key, _idx = candidates(raw_matrix, min_raw)
    parent = list(range(S))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    ti, tj = [], []
    for a, b in zip(ci.tolist(), cj.tolist()):
        if len(ti) == S - 1:
            break
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            ti.append(a)
            tj.append(b)
    component, n_comp = _labels(parent)
    return np.asarray(ti, dtype=np.int32), np.asarray(tj, dtype=np.int32), component, n_comp


def tied_competitors(raw_matrix, ti, tj, min_raw=None):
    """tree edges whose key some OTHER candidate edge shares: where the tie-break decided, or could have"""
    _ci, _cj, key, _idx = candidates(raw_matrix, min_raw)
    uniq, cnt = np.unique(key, return_counts=True)
    tree_key = sort_key(np.asarray(raw_matrix, dtype=np.float64)[ti, tj])
    return int(np.sum(cnt[np.searchsorted(uniq, tree_key)] > 1))


def verify_forest(raw_matrix, ti, tj, component, min_raw=None):
    """Independent of Kruskal, S <= 130: (1) the edges form a forest of candidate edges, (2) its components are those
    of the candidate graph and `component` numbers them by their smallest sample, (3) every candidate edge that is not
    in the forest is strictly worse in the order than every tree edge on the path between its ends (the cycle
    property, which with a total order characterises THE maximum spanning forest)."""
    raw_matrix = np.asarray(raw_matrix, dtype=np.float64)
    S = raw_matrix.shape[0]
    assert S <= 130
    ti, tj = np.asarray(ti, dtype=np.int64), np.asarray(tj, dtype=np.int64)
    assert np.all(ti < tj)
    ci, cj, _key, idx = candidates(raw_matrix, min_raw)
    rank = np.full((S, S), -1, dtype=np.int64)                # place in the strict order: smaller is better
    rank[ci, cj] = rank[cj, ci] = np.arange(len(idx))
    assert np.all(rank[ti, tj] >= 0), "a tree edge is no candidate"
    # (1) a forest: no edge closes a cycle
    parent = list(range(S))
    adj = [[] for _ in range(S)]
    for a, b in zip(ti.tolist(), tj.tolist()):
        ra, rb = a, b
        while parent[ra] != ra:
            ra = parent[ra]
        while parent[rb] != rb:
            rb = parent[rb]
        assert ra != rb, "the edges close a cycle"
        parent[ra] = rb
        adj[a].append(b)
        adj[b].append(a)
    # (2) the components of the candidate graph, by a search over its adjacency matrix
    cand = rank >= 0
    want = np.full(S, -1, dtype=np.int32)
    n_comp = 0
    for s in range(S):
        if want[s] >= 0:
            continue
        todo = [s]
        want[s] = n_comp
        while todo:
            a = todo.pop()
            for b in np.flatnonzero(cand[a] & (want < 0)).tolist():
                want[b] = n_comp
                todo.append(b)
        n_comp += 1
    forest_labels, forest_n = _labels(parent)
    assert forest_n == n_comp and np.array_equal(forest_labels, want)
    assert np.array_equal(np.asarray(component), want)
    assert len(ti) + n_comp == S
    # (3) the cycle property: the worst rank on the tree path from a to every b, by a walk over the tree from a
    in_tree = np.zeros((S, S), dtype=bool)
    in_tree[ti, tj] = in_tree[tj, ti] = True
    for a in range(S):
        worst = np.full(S, -1, dtype=np.int64)
        seen = np.zeros(S, dtype=bool)
        seen[a] = True
        todo = [a]
        while todo:
            u = todo.pop()
            for v in adj[u]:
                if not seen[v]:
                    seen[v] = True
                    worst[v] = max(worst[u], rank[u, v])
                    todo.append(v)
        others = cand[a] & ~in_tree[a]
        assert np.all(seen[others]), "a candidate edge joins two trees of the forest"
        assert np.all(rank[a][others] > worst[others]), "a non-tree edge beats a tree edge on its cycle"
    return n_comp
