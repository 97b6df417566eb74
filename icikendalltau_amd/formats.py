"""Input / output formats either side of the path.

* ``read_r_data(path)``: numeric matrices and vectors out of R's ``.rda`` / ``.RData`` / ``.rds`` files
  (XDR serialisation, gzip / bzip2 / xz / uncompressed), e.g. the reference's ``data/yeast_missing.rda``.
  A pure data reader: it understands the handful of SEXP types a numeric matrix with dimnames needs and
  evaluates nothing from the file.
* ``cor_matrix_2_long_df`` / ``long_df_2_cor_matrix``: the reference's converters between the square result
  matrices and the long data.frame storage form (R/reshaping.R:15-68).
* ``topk_to_csr``: the result of ``ici_kendalltau_topk`` as a sparse samples x samples kNN graph (needs scipy).
* ``cross_topk_to_csr``: the top-k lists of ``ici_kendalltau_cross`` as a sparse query x reference graph (needs scipy).
* ``edges_to_coo``: the result of ``ici_kendalltau_edges`` as a sparse samples x samples matrix (needs scipy).
* ``mst_to_linkage`` / ``mst_cut``: the result of ``ici_kendalltau_mst`` as a ``scipy.cluster.hierarchy`` linkage matrix
  (single linkage), and as the network's component labels at any cut-off (neither needs scipy).
* ``hclust_to_linkage`` / ``hclust_cut``: the result of ``ici_kendalltau_hclust`` (complete, average or single linkage)
  as a ``scipy.cluster.hierarchy`` linkage matrix, and as the clusters at any similarity (neither needs scipy).
"""
from __future__ import annotations

import bz2
import gzip
import lzma
import struct

import numpy as np

try:
    import pandas as pd
except Exception:  # pragma: no cover
    pd = None

# SEXP type codes of R's serialize.c
_NILVALUE, _REFSXP, _GLOBALENV, _EMPTYENV, _BASEENV, _MISSINGARG, _UNBOUND = 254, 255, 253, 242, 241, 251, 252
_SYMSXP, _LISTSXP, _CHARSXP, _LGLSXP, _INTSXP, _REALSXP, _STRSXP, _VECSXP = 1, 2, 9, 10, 13, 14, 16, 19
_ALTREP, _ATTRLISTSXP, _ATTRLANGSXP, _LANGSXP = 238, 239, 240, 6
_NA_INT = -2147483648


class RDataError(ValueError):
    pass


class _Reader:
    def __init__(self, buf: bytes):
        self.b = buf
        self.p = 0
        self.refs = []

    def take(self, n: int) -> bytes:
        if self.p + n > len(self.b):
            raise RDataError("truncated R data stream")
        out = self.b[self.p:self.p + n]
        self.p += n
        return out

    def i32(self) -> int:
        return struct.unpack(">i", self.take(4))[0]

    def length(self) -> int:
        n = self.i32()
        if n == -1:  # long vector: two more ints
            hi, lo = struct.unpack(">II", self.take(8))
            n = (hi << 32) | lo
        return n

    def item(self):
        flags = self.i32()
        t = flags & 0xFF
        has_attr = bool(flags & 0x200)
        has_tag = bool(flags & 0x400)
        if t in (_NILVALUE, _GLOBALENV, _EMPTYENV, _BASEENV, _MISSINGARG, _UNBOUND):
            return None
        if t == _REFSXP:
            idx = flags >> 8
            if idx == 0:
                idx = self.i32()
            return self.refs[idx - 1]
        if t == _SYMSXP:
            name = self.item()
            self.refs.append(name)
            return name
        if t == _CHARSXP:
            n = self.i32()
            return None if n == -1 else self.take(n).decode("utf-8", "replace")
        if t in (_LISTSXP, _LANGSXP, _ATTRLISTSXP, _ATTRLANGSXP):
            # pairlist: [attr] [tag] car cdr ; returned as a list of (tag, value)
            out = []
            while True:
                if t in (_ATTRLISTSXP, _ATTRLANGSXP) or has_attr:
                    self.item()
                tag = self.item() if has_tag else None
                out.append((tag, self.item()))
                flags = self.i32()
                t = flags & 0xFF
                has_attr = bool(flags & 0x200)
                has_tag = bool(flags & 0x400)
                if t == _NILVALUE:
                    return out
                if t not in (_LISTSXP, _LANGSXP, _ATTRLISTSXP, _ATTRLANGSXP):
                    raise RDataError(f"unsupported pairlist tail type {t}")
        if t in (_LGLSXP, _INTSXP):
            n = self.length()
            v = np.frombuffer(self.take(4 * n), dtype=">i4").astype(np.int32)
            return self._with_attr(v, has_attr, logical=(t == _LGLSXP))
        if t == _REALSXP:
            n = self.length()
            v = np.frombuffer(self.take(8 * n), dtype=">f8").astype(np.float64)
            return self._with_attr(v, has_attr)
        if t == _STRSXP:
            n = self.length()
            v = [self.item() for _ in range(n)]
            return self._with_attr(v, has_attr)
        if t == _VECSXP:
            n = self.length()
            v = [self.item() for _ in range(n)]
            return self._with_attr(v, has_attr)
        if t == _ALTREP:
            info = self.item()       # pairlist: class symbol, package symbol, type
            state = self.item()
            self.item()              # attributes
            cls = info[0][1] if info else None
            if cls in ("compact_intseq", "compact_realseq"):
                n, start, step = (float(x) for x in np.asarray(state)[:3])
                return start + step * np.arange(int(n))
            if cls in ("wrap_real", "wrap_integer", "wrap_logical", "wrap_string"):
                return state[0] if isinstance(state, list) else state
            raise RDataError(f"unsupported ALTREP class {cls!r}")
        raise RDataError(f"unsupported R object type {t}")

    def _with_attr(self, value, has_attr, logical=False):
        attrs = {}
        if has_attr:
            for tag, val in (self.item() or []):
                attrs[tag] = val
        return {"value": value, "attr": attrs, "logical": logical} if attrs or logical else value


def _decompress(raw: bytes) -> bytes:
    if raw[:2] == b"\x1f\x8b":
        return gzip.decompress(raw)
    if raw[:3] == b"BZh":
        return bz2.decompress(raw)
    if raw[:6] == b"\xfd7zXZ\x00":
        return lzma.decompress(raw)
    return raw


def _to_numpy(obj):
    """R object -> ndarray (matrix with names) where it is numeric; NA_integer_ / NA_logical_ -> NaN."""
    if isinstance(obj, dict):
        v, attrs = obj["value"], obj["attr"]
        if isinstance(v, np.ndarray):
            if v.dtype == np.int32:
                v = np.where(v == _NA_INT, np.nan, v.astype(np.float64))
            dim = attrs.get("dim")
            if dim is not None:
                d = np.asarray(dim["value"] if isinstance(dim, dict) else dim, dtype=np.int64)
                v = np.asfortranarray(v.reshape(tuple(int(x) for x in d), order="F"))
            names = attrs.get("dimnames") or attrs.get("names")
            return {"data": v, "dimnames": names}
        return {"data": v, "attr": attrs}
    if isinstance(obj, np.ndarray) and obj.dtype == np.int32:
        return {"data": np.where(obj == _NA_INT, np.nan, obj.astype(np.float64)), "dimnames": None}
    return {"data": obj, "dimnames": None}


def read_r_data(path: str) -> dict:
    """Objects of an .rda/.RData file (name -> {"data": ndarray, "dimnames": ...}) or the single object of
    an .rds file (under the key None)."""
    buf = _decompress(open(path, "rb").read())
    is_rda = buf[:4] in (b"RDX2", b"RDX3")
    if is_rda:
        buf = buf[5:]
    if buf[:2] != b"X\n":
        raise RDataError("only the XDR serialisation format is supported")
    r = _Reader(buf)
    r.take(2)
    version = r.i32()
    r.i32()
    r.i32()
    if version == 3:
        r.take(r.i32())  # native encoding name
    elif version != 2:
        raise RDataError(f"unsupported serialisation version {version}")
    top = r.item()
    if is_rda:
        return {tag: _to_numpy(val) for tag, val in top}
    return {None: _to_numpy(top)}


def read_r_matrix(path: str, name: str | None = None):
    """(matrix, rownames, colnames) of the (named or only) numeric matrix in an R data file."""
    objs = read_r_data(path)
    if name is None:
        cands = [k for k, v in objs.items() if isinstance(v.get("data"), np.ndarray) and v["data"].ndim == 2]
        if len(cands) != 1:
            raise RDataError(f"expected exactly one matrix, found {cands}")
        name = cands[0]
    obj = objs[name]
    dn = obj.get("dimnames")
    rn = cn = None
    if isinstance(dn, list) and len(dn) == 2:
        rn, cn = dn
        rn = rn["value"] if isinstance(rn, dict) else rn
        cn = cn["value"] if isinstance(cn, dict) else cn
    return obj["data"], rn, cn


# --------------------------------------------------------------------------------------------------
# R/reshaping.R
# --------------------------------------------------------------------------------------------------
def cor_matrix_2_long_df(in_matrix):
    """Square matrix (DataFrame with row / column names) -> long data.frame(s1, s2, cor), stacked column by
    column as utils::stack does (R/reshaping.R:15-32)."""
    if pd is None:
        raise RuntimeError("pandas is required")
    df = in_matrix if isinstance(in_matrix, pd.DataFrame) else pd.DataFrame(in_matrix)
    vals = df.to_numpy()
    rows = np.asarray([str(r) for r in df.index], dtype=object)
    cols = np.asarray([str(c) for c in df.columns], dtype=object)
    return pd.DataFrame({"s1": np.tile(rows, len(cols)), "s2": np.repeat(cols, len(rows)),
                         "cor": vals.reshape(-1, order="F")})


def long_df_2_cor_matrix(long_df, is_square=True):
    """long data.frame(s1, s2, cor) -> (possibly square) matrix; half-filled square input is mirrored
    (R/reshaping.R:44-68).  Levels are sorted, as factor() sorts them."""
    if pd is None:
        raise RuntimeError("pandas is required")
    if not all(c in long_df.columns for c in ("s1", "s2", "cor")):
        raise ValueError("The data.frame must contain the names 's1', 's2', and 'cor'.")
    s1 = long_df["s1"].astype(str).to_numpy()
    s2 = long_df["s2"].astype(str).to_numpy()
    if is_square:
        l1 = l2 = sorted(set(s1) | set(s2))
    else:
        l1, l2 = sorted(set(s1)), sorted(set(s2))
    i1 = {k: i for i, k in enumerate(l1)}
    i2 = {k: i for i, k in enumerate(l2)}
    m = np.full((len(l1), len(l2)), np.nan)
    r = np.fromiter((i1[a] for a in s1), dtype=np.int64, count=len(s1))
    c = np.fromiter((i2[b] for b in s2), dtype=np.int64, count=len(s2))
    vals = long_df["cor"].to_numpy(dtype=np.float64)
    m[r, c] = vals
    if len(long_df) != m.shape[0] * m.shape[1] and is_square:
        m[c, r] = vals
    return pd.DataFrame(m, index=l1, columns=l2)


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_topk -> a sparse kNN graph
# --------------------------------------------------------------------------------------------------
def topk_to_csr(result, value="cor"):
    """The dict ``ici_kendalltau_topk`` returns as an S x S ``scipy.sparse.csr_matrix``: row s holds ``result[value]``
    of sample s's partners at their column indices (in the list's order); padded slots are dropped, so the matrix has
    ``sum(n_valid)`` stored entries.  scipy is optional for the package and needed here."""
    try:
        import scipy.sparse as sp
    except ImportError as e:
        raise ImportError("topk_to_csr needs scipy (optional for icikendalltau_amd, required for this converter)") from e
    if value not in ("cor", "raw", "pvalue", "taumax", "completeness"):
        raise ValueError("`value` must be one of cor, raw, pvalue, taumax, completeness")
    idx = np.asarray(result["indices"])
    vals = np.asarray(result[value], dtype=np.float64)
    n_valid = np.asarray(result["n_valid"], dtype=np.int64)
    S, k = idx.shape
    real = np.arange(k)[None, :] < n_valid[:, None]
    indptr = np.concatenate([[0], np.cumsum(n_valid)])
    return sp.csr_matrix((vals[real], idx[real].astype(np.int32), indptr), shape=(S, S))


def cross_topk_to_csr(result, value="cor", n_reference=None):
    """The top-k part of the dict ``ici_kendalltau_cross`` returns (called with ``k``) as an Sq x Sr
    ``scipy.sparse.csr_matrix``: row q holds ``result[value]`` of query q's partners at their reference column indices
    (in the list's order); padded slots are dropped, so the matrix has ``sum(n_valid)`` stored entries.  Sr is taken from
    ``result["reference_names"]`` unless ``n_reference`` gives it.  scipy is optional for the package and needed
    here."""
    try:
        import scipy.sparse as sp
    except ImportError as e:
        raise ImportError("cross_topk_to_csr needs scipy (optional for icikendalltau_amd, required for this converter)") from e
    if value not in ("cor", "raw", "pvalue", "taumax", "completeness"):
        raise ValueError("`value` must be one of cor, raw, pvalue, taumax, completeness")
    if "indices" not in result:
        raise ValueError("the result holds no top-k lists: call ici_kendalltau_cross with `k`")
    idx = np.asarray(result["indices"])
    vals = np.asarray(result["topk_" + value], dtype=np.float64)
    n_valid = np.asarray(result["n_valid"], dtype=np.int64)
    Sq, k = idx.shape
    Sr = int(n_reference) if n_reference is not None else len(result["reference_names"])
    real = np.arange(k)[None, :] < n_valid[:, None]
    indptr = np.concatenate([[0], np.cumsum(n_valid)])
    return sp.csr_matrix((vals[real], idx[real].astype(np.int32), indptr), shape=(Sq, Sr))


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_edges -> a sparse correlation network
# --------------------------------------------------------------------------------------------------
def edges_to_coo(result, value="cor", symmetric=True):
    """The dict ``ici_kendalltau_edges`` returns as an S x S ``scipy.sparse.coo_matrix`` of ``result[value]``: every
    edge at (i, j) and, with ``symmetric``, at (j, i) as well (the upper triangle alone otherwise); the diagonal is
    empty.  S is the length of ``result["degree"]``.  scipy is optional for the package and needed here."""
    try:
        import scipy.sparse as sp
    except ImportError as e:
        raise ImportError("edges_to_coo needs scipy (optional for icikendalltau_amd, required for this converter)") from e
    if value not in ("cor", "raw", "pvalue", "taumax", "completeness"):
        raise ValueError("`value` must be one of cor, raw, pvalue, taumax, completeness")
    S = len(result["degree"])
    i = np.asarray(result["i"], dtype=np.int32)
    j = np.asarray(result["j"], dtype=np.int32)
    vals = np.asarray(result[value], dtype=np.float64)
    if symmetric:
        i, j, vals = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([vals, vals])
    return sp.coo_matrix((vals, (i, j)), shape=(S, S))


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_mst -> a dendrogram, and the network's components at any cut-off
# --------------------------------------------------------------------------------------------------
def _mst_find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def mst_to_linkage(result, by="raw"):
    """The dict ``ici_kendalltau_mst`` returns as a ``scipy.cluster.hierarchy`` linkage matrix of single linkage under
    the distance ``1 - result[by]`` (``by``: "raw" or "cor"): (S - 1) x 4 float64, row k = (the two clusters merged at
    step k, the smaller id first; the height ``1 - value`` of the tree's k-th edge; the new cluster's size), the samples
    being clusters 0 .. S - 1 and step k making cluster S + k -- scipy's convention, so ``dendrogram``, ``fcluster`` and
    ``leaves_list`` take it as it is.  The tree's edges come in the single-linkage merge order, so this is one pass of
    union-find, O(S alpha(S)); scipy itself is not needed.  A forest that is not ONE tree has no dendrogram:
    ``ValueError`` naming ``n_components`` (cut with ``mst_cut``, or cluster each component on its own)."""
    if by not in ("raw", "cor"):
        raise ValueError("`by` must be raw or cor")
    S = len(result["component"])
    n_comp = int(result["n_components"])
    i = np.asarray(result["i"], dtype=np.int64)
    j = np.asarray(result["j"], dtype=np.int64)
    if n_comp != 1 or i.shape[0] != S - 1:
        raise ValueError(f"the forest is not one tree (n_components = {n_comp}): a linkage matrix needs every sample "
                         "connected; lower `min_raw`, or cut with mst_cut")
    height = 1.0 - np.asarray(result[by], dtype=np.float64)
    parent = list(range(S))
    cluster = list(range(S))     # per union-find root: the id of the cluster it stands for
    size = [1] * S
    Z = np.empty((S - 1, 4), dtype=np.float64)
    for k in range(S - 1):
        a, b = _mst_find(parent, int(i[k])), _mst_find(parent, int(j[k]))
        if a == b:
            raise ValueError(f"edge {k} of the result closes a cycle: not a forest of ici_kendalltau_mst")
        ca, cb = cluster[a], cluster[b]
        parent[b] = a
        size[a] += size[b]
        cluster[a] = S + k
        Z[k] = (min(ca, cb), max(ca, cb), height[k], size[a])
    return Z


def mst_cut(result, min_raw):
    """The connected components of the network "every pair with ``raw >= min_raw``" from the tree alone: the tree's edges
    below ``min_raw`` are dropped and the rest merged by union-find (a maximum spanning forest connects, at every
    cut-off, exactly what the full graph connects).  ``result``: the dict of ``ici_kendalltau_mst`` called with no
    ``min_raw``, or with one not above this one.  Returns the labels (S, int32), numbered 0, 1, ... in order of each
    component's smallest sample: ``ici_kendalltau_mst(..., min_raw=min_raw)["component"]`` without computing a pair."""
    S = len(result["component"])
    i = np.asarray(result["i"], dtype=np.int64)
    j = np.asarray(result["j"], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        keep = np.asarray(result["raw"], dtype=np.float64) >= float(min_raw)
    parent = list(range(S))
    for a, b in zip(i[keep].tolist(), j[keep].tolist()):
        a, b = _mst_find(parent, a), _mst_find(parent, b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    label = np.full(S, -1, dtype=np.int32)
    component = np.empty(S, dtype=np.int32)
    n = 0
    for s in range(S):
        r = _mst_find(parent, s)
        if label[r] < 0:
            label[r] = n
            n += 1
        component[s] = label[r]
    return component


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_hclust -> a dendrogram, and the clusters at any similarity
# --------------------------------------------------------------------------------------------------
def hclust_to_linkage(result, by="raw"):
    """The dict ``ici_kendalltau_hclust`` returns as a ``scipy.cluster.hierarchy`` linkage matrix under the distance
    ``1 - result[by]`` (``by``: "raw" or "cor"): (S - 1) x 4 float64, row k = (the two clusters merged at step k, the
    smaller id first; the height ``1 - value`` of the merge; the new cluster's size), the samples being clusters
    0 .. S - 1 and step k making cluster S + k -- scipy's numbering, so ``dendrogram``, ``fcluster`` and
    ``leaves_list`` take it as it is.  One pass over the merges, O(S); scipy itself is not needed.  Complete and single
    linkage only take minima and maxima, so their heights never decrease.  Average linkage on similarities is
    monotone in exact arithmetic; each of its updates rounds, so a height can in principle come out below the one
    before it by an ulp or so.  Nothing is clamped: the heights are the similarities the merges were made at.
    A forest that is not ONE tree has no dendrogram: ``ValueError`` naming ``n_components`` (cut with ``hclust_cut``,
    or cluster each component on its own)."""
    if by not in ("raw", "cor"):
        raise ValueError("`by` must be raw or cor")
    S = len(result["component"])
    n_comp = int(result["n_components"])
    a = np.asarray(result["merge_a"], dtype=np.int64)
    b = np.asarray(result["merge_b"], dtype=np.int64)
    if n_comp != 1 or a.shape[0] != S - 1:
        raise ValueError(f"the result is a forest, not one tree (n_components = {n_comp}): a linkage matrix needs every "
                         "sample merged; lower `min_raw`, or cut with hclust_cut")
    height = 1.0 - np.asarray(result[by], dtype=np.float64)
    size = np.asarray(result["size"], dtype=np.int64)
    cluster = list(range(S))     # per slot: the id of the cluster that lives in it
    alive = [True] * S
    Z = np.empty((S - 1, 4), dtype=np.float64)
    for k in range(S - 1):
        sa, sb = int(a[k]), int(b[k])
        if not (0 <= sa < sb < S and alive[sa] and alive[sb]):
            raise ValueError(f"merge {k} of the result names a slot that is no cluster: not a result of ici_kendalltau_hclust")
        ca, cb = cluster[sa], cluster[sb]
        alive[sb] = False
        cluster[sa] = S + k
        Z[k] = (min(ca, cb), max(ca, cb), height[k], size[k])
    return Z


def hclust_cut(result, min_raw):
    """The clusters at the similarity ``min_raw`` from the merges alone: the merges are replayed up to the first one whose
    ``raw`` is below ``min_raw`` (NA compares as below), which is where ``ici_kendalltau_hclust(..., min_raw=min_raw)``
    ends.  ``result``: the dict of ``ici_kendalltau_hclust`` called with no ``min_raw``, or with one not above this one.
    Returns the labels (S, int32), numbered 0, 1, ... in order of each cluster's smallest sample: that call's
    ``component`` without computing a pair."""
    S = len(result["component"])
    a = np.asarray(result["merge_a"], dtype=np.int64)
    b = np.asarray(result["merge_b"], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        keep = np.asarray(result["raw"], dtype=np.float64) >= float(min_raw)
    n = int(np.argmin(keep)) if not np.all(keep) else int(keep.shape[0])
    slot = np.arange(S)          # the slot a sample's cluster lives in: a slot merges into a smaller one, so one ascending pass resolves them
    for sa, sb in zip(a[:n].tolist(), b[:n].tolist()):
        slot[sb] = sa
    label = np.full(S, -1, dtype=np.int32)
    component = np.empty(S, dtype=np.int32)
    k = 0
    for s in range(S):
        if slot[s] == s:
            label[s] = k
            k += 1
        else:
            slot[s] = slot[slot[s]]
        component[s] = label[slot[s]]
    return component
