"""Compressed-sparse-column input (icikt_csc_input) on the MI355X: k_scatter_csc alone through Context.scatter_csc_dev,
every *_csc entry against its _in twin, the chunked and pipelined routes, the argument errors and the front ends.

The reference everywhere is the existing dense route on A.toarray() with `fill` put in: icikt_convert_dev's float64 matrix
for the kernel, the _in entries for everything else (tests/test_gpu_ingest.py and the parity tests pin that route).  The
device matrix a CSC view leaves behind is that float64 matrix bit for bit and nothing behind it differs, so every output
-- integers and doubles -- is compared for equality through a uint64 view (NaN equal to NaN, payloads included)."""
import ctypes
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib

sp = pytest.importorskip("scipy.sparse")

pytestmark = pytest.mark.gpu

NP_DTYPES = {_lib.DTYPE_F64: np.float64, _lib.DTYPE_F32: np.float32, _lib.DTYPE_I32: np.int32, _lib.DTYPE_I64: np.int64}
NP_INDEX = {_lib.INDEX_I32: np.int32, _lib.INDEX_I64: np.int64}
NA_REAL_BITS = 0x7FF00000000007A2
SENTINEL = -12345.678
GNA = (np.nan, np.inf, 0)


def f64_bits(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


FILLS = [f64_bits(0), f64_bits(0x8000000000000000), f64_bits(NA_REAL_BITS), 7.5]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the kernel alone ------------------------------------------------------------------------------------------------

def special_values(code):
    """tests/test_gpu_ingest.py::special_values, by value"""
    if code == _lib.DTYPE_F64:
        bits = [NA_REAL_BITS, 0x7FF8000000000000, 0xFFF8000000000BAD, 0x7FF0000000000000, 0xFFF0000000000000,
                0x8000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF]
        return np.array(bits, dtype=np.uint64).view(np.float64)
    if code == _lib.DTYPE_F32:
        bits = [0x7FC00000, 0xFFC00123, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000,
                0x007FFFFF, 0x00000001, 0x807FFFFF, 0x7F7FFFFF]
        return np.array(bits, dtype=np.uint32).view(np.float32)
    if code == _lib.DTYPE_I32:
        return np.array([-2**31, 2**31 - 1, 0, -1, 16777217], dtype=np.int32)
    return np.array([2**53 + 1, -(2**53 + 1), -2**63, 2**63 - 1, 2**53 + 3, 2**62 + 1, 0, -1], dtype=np.int64)


def random_csc(rng, code, itype, n, S, density, special=True):
    """(data, indices, indptr, D, present): a CSC matrix built by hand -- indices shuffled within every column, one empty
    and one full column where the shape has room, the dtype's special values and an explicitly stored 0 among the
    entries -- and the dense matrix D of the same dtype (absent cells 0) with the mask of the cells that have an entry"""
    dt = NP_DTYPES[code]
    present = rng.random((n, S)) < density
    if S >= 3:
        present[:, S // 2] = False
    if S >= 2:
        present[:, S - 1] = True
    if code in (_lib.DTYPE_F64, _lib.DTYPE_F32):
        D = rng.standard_normal((n, S)).astype(dt)
    else:
        D = rng.integers(1, 10**6, size=(n, S)).astype(dt)
    D = np.asfortranarray(D)
    D[~present] = 0
    rr, cc = np.nonzero(present)
    if special and rr.size:
        spv = np.concatenate([special_values(code), np.zeros(1, dtype=dt)])     # (... and an explicitly stored 0)
        k = min(spv.size, rr.size)
        pick = rng.permutation(rr.size)[:k]
        D[rr[pick], cc[pick]] = spv[:k]
    cols, rows = np.nonzero(present.T)                      # column by column, rows ascending ...
    order = np.lexsort((rng.random(rows.size), cols))       # ... then shuffled within every column
    rows, cols = rows[order], cols[order]
    data = np.ascontiguousarray(D[rows, cols])
    indptr = np.concatenate(([0], np.cumsum(present.sum(axis=0)))).astype(NP_INDEX[itype])
    return data, rows.astype(NP_INDEX[itype]), indptr, D, present


class ScatterCase:
    """A CSC matrix on the device and its reference: icikt_convert_dev's float64 matrix of the dense block, computed once;
    `fill` is put into the absent cells per check"""

    def __init__(self, ctx, rng, code, itype, n, S, density, special=True):
        import torch
        self.ctx, self.code, self.itype, self.n, self.S = ctx, code, itype, n, S
        data, indices, indptr, D, present = random_csc(rng, code, itype, n, S, density, special)
        self.nnz = data.size
        self.d = [torch.from_numpy(a).cuda() for a in (data, indices, indptr)]
        d_src = torch.from_numpy(D.T.copy()).cuda()           # row j = column j: column-major with ld = n
        d_ref = torch.empty((S, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.convert_dev(d_src.data_ptr(), code, _lib.ORDER_COL, n, S, n, d_ref.data_ptr(), n)
        ctx.sync()
        self.ref = d_ref.cpu().numpy()
        self.absent = ~present.T

    def check(self, fill, dst_pad):
        import torch
        n, S = self.n, self.S
        dst_ld = n + dst_pad
        d_dst = torch.full((S, dst_ld), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()                              # (the fill runs on torch's stream, the scatter on the context's)
        self.ctx.scatter_csc_dev(self.d[0].data_ptr(), self.d[1].data_ptr(), self.d[2].data_ptr(), self.code, self.itype,
                                 fill, n, S, d_dst.data_ptr(), dst_ld)
        got = d_dst.cpu().numpy()
        label = (self.code, self.itype, n, S, float(fill), dst_pad)
        assert np.all(got[:, n:] == SENTINEL), label          # rows [n, dst_ld) of every column are untouched
        want = self.ref.copy()
        want.view(np.uint64)[self.absent] = np.array([fill], dtype=np.float64).view(np.uint64)[0]
        assert bits_equal(got[:, :n], want), label


SHAPES = [(1, 1), (1, 200), (200, 1), (63, 65), (64, 64), (65, 63), (257, 3), (1025, 5)]


@pytest.mark.parametrize("itype", sorted(NP_INDEX))
@pytest.mark.parametrize("code", sorted(NP_DTYPES))
def test_scatter_csc_dev_shapes_values_and_fills(hip_ctx, code, itype):
    rng = np.random.default_rng(10 * code + itype)
    for n, S in SHAPES:
        case = ScatterCase(hip_ctx, rng, code, itype, n, S, 0.1)
        for fill in FILLS:
            for dst_pad in (0, 3):
                case.check(fill, dst_pad)
    empty = ScatterCase(hip_ctx, rng, code, itype, 65, 2, 0.0, special=False)      # nnz = 0 but for ...
    assert empty.nnz == 65                                                         # ... the full column; and none at all:
    import torch
    d_dst = torch.full((4, 70), SENTINEL, dtype=torch.float64, device="cuda")
    d_ptr = torch.zeros(5, dtype=torch.int32 if itype == _lib.INDEX_I32 else torch.int64, device="cuda")
    torch.cuda.synchronize()
    hip_ctx.scatter_csc_dev(0, 0, d_ptr.data_ptr(), code, itype, 7.5, 67, 4, d_dst.data_ptr(), 70)
    got = d_dst.cpu().numpy()
    assert np.all(got[:, :67] == 7.5) and np.all(got[:, 67:] == SENTINEL)
    empty.check(FILLS[2], 3)


@pytest.mark.parametrize("code,itype", [(_lib.DTYPE_F32, _lib.INDEX_I32), (_lib.DTYPE_F64, _lib.INDEX_I64)])
@pytest.mark.parametrize("n,S", [(3, 70000), (65537, 3), (262144, 3)])
def test_scatter_csc_dev_past_the_caps(hip_ctx, n, S, code, itype):
    """More columns than a launch has workgroups (1 024: icikt_sparse.hip), so workgroups take further rounds of the
    grid-stride loop; 65 537 and 262 144 rows: the LDS bitset past 8 KB and at its largest (32 KB)."""
    case = ScatterCase(hip_ctx, np.random.default_rng(n + code), code, itype, n, S, 0.05)
    case.check(FILLS[2], 2)
    case.check(FILLS[0], 0)


# ---- every *_csc entry against its _in twin ------------------------------------------------------------------------------

def count_like(n=300, S=7, seed=11, dtype=np.float32):
    """integers 0 .. 30, 60 % zeros, a few NaN entries"""
    rng = np.random.default_rng(seed)
    M = rng.integers(1, 31, size=(n, S)).astype(dtype)
    M[rng.random((n, S)) < 0.6] = 0
    M[rng.random((n, S)) < 0.01] = np.nan
    return M


def dense_with_fill(A, fill=0.0):
    """A.toarray() with `fill` put into the cells that have no entry (stored zeros are entries)"""
    A = A.tocsc()
    D = np.asfortranarray(A.toarray())
    B = A.copy()
    B.data = np.ones_like(B.data)
    D[B.toarray() == 0] = fill
    return D


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (int, np.integer)):
        return int(a) == int(b)
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        return bits_equal(a, b)
    return np.array_equal(a, b)


def run_csc_entries(ctx, X, S):
    out = {}
    cls = (np.arange(S) % 2).astype(np.int32)
    for persp in ("global", "local"):
        out["pairs " + persp] = ctx.pairs(X, perspective=persp, want_counts=True)
    for scale_max in (True, False):
        for diag_good in (True, False):
            pi, pj = (None, None) if diag_good else [a.astype(np.int32) for a in np.triu_indices(S, k=0)]
            out[f"matrix {scale_max} {diag_good}"] = ctx.matrix(X, global_na=GNA, pi=pi, pj=pj, scale_max=scale_max,
                                                                diag_good=diag_good, want_keep=True)
    pi, pj = [a.astype(np.int32) for a in np.triu_indices(S, k=0)]
    out["missingness"] = (ctx.missingness(X, pi, pj),)
    out["col_medians"] = (ctx.col_medians(X, na_rm=False, global_na=GNA), ctx.col_medians(X, na_rm=True, global_na=GNA),
                          ctx.col_medians(X, na_rm=True))
    out["censor_counts"] = ctx.censor_counts(X, GNA, cls, 2, want_medians=True)
    for label, cols in (("consecutive", np.arange(2, S, dtype=np.int32)), ("gathered", np.array([5, 0, 3, 6], dtype=np.int32))):
        r = ctx.rank_order(X, GNA, cols)
        out["rank_order " + label] = tuple(r[k] for k in sorted(r))
    return out


def assert_same_outputs(got, ref, label):
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert len(got[name]) == len(ref[name]), (label, name)
        for k, (g, r) in enumerate(zip(got[name], ref[name])):
            assert same(g, r), (label, name, k)


@pytest.mark.parametrize("dtype,itype", [(np.float32, np.int32), (np.float64, np.int64)])
@pytest.mark.parametrize("fill", [0.0, np.nan])
def test_csc_entries_equal_their_in_twins(hip_ctx, fill, dtype, itype):
    A = sp.csc_matrix(count_like(dtype=dtype))
    A.indices, A.indptr = A.indices.astype(itype), A.indptr.astype(itype)
    S = A.shape[1]
    view = _lib.csc_view(A, fill=fill)
    assert view.copied is False
    D = dense_with_fill(A, fill)
    assert bits_equal(view.toarray(), D.astype(np.float64))
    assert_same_outputs(run_csc_entries(hip_ctx, view, S), run_csc_entries(hip_ctx, D, S), (fill, dtype))
    if fill == 0.0:                                           # a scipy matrix directly: fill 0
        assert_same_outputs(run_csc_entries(hip_ctx, A, S), run_csc_entries(hip_ctx, D, S), "scipy")


# ---- chunked and pipelined routes ------------------------------------------------------------------------------------------

BIG_N, BIG_S = 4099, 800          # 26 MB as float64: four 8 MB chunks of 254 columns, above the 24 MB pipeline threshold


@pytest.fixture(scope="module")
def big(hip_ctx):
    """(A, D, reference outputs of the dense _in call): density 0.02, float32 / int32; columns [254, 508) -- the second
    chunk -- hold no entry at all"""
    rng = np.random.default_rng(4099)
    M = rng.integers(1, 200, size=(BIG_N, BIG_S)).astype(np.float32)
    M[rng.random((BIG_N, BIG_S)) >= 0.02] = 0
    M[:, 254:508] = 0
    A = sp.csc_matrix(M)
    assert A.indptr[254] == A.indptr[508] and A.nnz * 8 > 256 * 1024 and A.indices.dtype == np.int32
    D = np.asfortranarray(M)
    ref = hip_ctx.pairs(D, perspective="global", want_counts=True)
    return A, D, ref


@pytest.mark.parametrize("plan", ["pipe=0", "pipe=1", "pipe=1,merge=0"])
def test_pairs_csc_chunked_and_pipelined(plan_ctx, big, plan):
    A, _D, ref = big
    plan_ctx.debug_set_plan(plan)
    got = plan_ctx.pairs(A, perspective="global", want_counts=True)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert same(g, r), (plan, k)


def test_pairs_csc_from_caller_pinned_arrays(hip_ctx, big):
    A, _D, ref = big
    data = _lib.pinned_empty(A.nnz, dtype=np.float32)
    indices = _lib.pinned_empty(A.nnz, dtype=np.int32)
    data[...] = A.data
    indices[...] = A.indices
    view = _lib.CscView(data, indices, A.indptr, A.shape, 0.0, copied=False)
    got = hip_ctx.pairs(view, perspective="global", want_counts=True, flags=_lib.FLAG_HOST_PINNED)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert same(g, r), k


# ---- argument errors ---------------------------------------------------------------------------------------------------------

def raw_pairs_csc(ctx, struct, n, S):
    """icikt_pairs_csc on a raw icikt_csc_input (or none): (status, message, out4)"""
    L = _lib.lib()
    P = S * (S - 1) // 2
    out4 = np.full((P, 4), 7.0)
    rc = L.icikt_pairs_csc(ctx._h, None if struct is None else ctypes.byref(struct), n, S, None, None, 0, 1, 0, 0, 0,
                           out4.ctypes.data, None, None)
    return rc, L.icikt_last_error(ctx._h).decode(), out4


def test_csc_argument_errors(hip_ctx, big):
    ctx = hip_ctx
    n, S = 5, 3
    M = np.array([[1, 0, 2], [0, 3, 0], [4, 0, 5], [0, 6, 0], [7, 8, 9]], dtype=np.float32)
    good = _lib.csc_view(sp.csc_matrix(M))
    want = ctx.pairs(np.asfortranarray(M), perspective="global", want_counts=False)[0]

    def still_computes():
        rc, _msg, out4 = raw_pairs_csc(ctx, good.struct(), n, S)
        assert rc == 0 and bits_equal(out4, want)

    def variant(**kw):
        a = {"data": good.data.copy(), "indices": good.indices.copy(), "indptr": good.indptr.copy()}
        a.update(kw)
        return _lib.CscView(a["data"], a["indices"], a["indptr"], (n, S), 0.0, copied=True)

    def struct_of(view, **fields):
        s = view.struct()
        for k, v in fields.items():
            setattr(s, k, v)
        return view, s

    ip = good.indptr
    idx_hi, idx_neg, idx_dup = good.indices.copy(), good.indices.copy(), good.indices.copy()
    idx_hi[ip[1]] = n                                         # the first entry of column 1
    idx_neg[ip[2] - 1] = -1                                   # the last entry of column 1
    idx_dup[ip[2] + 1] = idx_dup[ip[2]]                       # column 2: two entries of one row
    dec = ip.copy()
    dec[1], dec[2] = ip[2], ip[1]
    neg0 = ip.copy()
    neg0[0] = -1
    cases = {
        "null view": ((None, None), "null"),
        "null values": (struct_of(good, values=None), "values"),
        "null indices": (struct_of(good, indices=None), "indices"),
        "dtype 7": (struct_of(good, dtype=7), "dtype"),
        "dtype -1": (struct_of(good, dtype=-1), "dtype"),
        "index_type 2": (struct_of(good, index_type=2), "index_type"),
        "indptr[0] = -1": (struct_of(variant(indptr=neg0)), "indptr[0]"),
        "decreasing indptr": (struct_of(variant(indptr=dec)), "indptr decreases"),
        "index = n_feat": (struct_of(variant(indices=idx_hi)), "outside [0, n_feat)"),
        "index = -1": (struct_of(variant(indices=idx_neg)), "outside [0, n_feat)"),
        "duplicate": (struct_of(variant(indices=idx_dup)), "duplicate entry (sum_duplicates)"),
    }
    for what, ((_keep, s), needle) in cases.items():
        rc, msg, _out4 = raw_pairs_csc(ctx, s, n, S)
        assert rc == -1 and needle in msg, (what, rc, msg)
        still_computes()
    # the device-side checks through the other entries and the device entry
    import torch
    for what, idx in (("index = n_feat", idx_hi), ("index = -1", idx_neg), ("duplicate", idx_dup)):
        bad = variant(indices=idx)
        for call in (lambda: ctx.matrix(bad, global_na=GNA), lambda: ctx.col_medians(bad, na_rm=True),
                     lambda: ctx.censor_counts(bad, GNA, np.zeros(S, dtype=np.int32), 1),
                     lambda: ctx.missingness(bad, np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)),
                     lambda: ctx.rank_order(bad, GNA, np.arange(S, dtype=np.int32)),
                     lambda: ctx.rank_order(bad, GNA, np.array([2, 1], dtype=np.int32))):
            with pytest.raises(_lib.IciktError, match=r"code -1.*(outside \[0, n_feat\)|duplicate entry \(sum_duplicates\))"):
                call()
            still_computes()
        d = [torch.from_numpy(a).cuda() for a in (bad.data, bad.indices, bad.indptr)]
        d_dst = torch.full((S, n), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(_lib.IciktError, match=r"code -1.*(outside \[0, n_feat\)|duplicate entry \(sum_duplicates\))"):
            ctx.scatter_csc_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), _lib.DTYPE_F32, _lib.INDEX_I32, 0.0, n, S,
                                d_dst.data_ptr(), n)
        still_computes()
    d_ptr = torch.from_numpy(dec).cuda()
    with pytest.raises(_lib.IciktError, match=r"code -1.*indptr decreases"):
        ctx.scatter_csc_dev(d[0].data_ptr(), d[1].data_ptr(), d_ptr.data_ptr(), _lib.DTYPE_F32, _lib.INDEX_I32, 0.0, n, S,
                            d_dst.data_ptr(), n)
    # a duplicate deep inside the multi-chunk shape: the last chunk, staged route, every plan
    A, _D, ref = big
    idx = A.indices.copy()
    c = BIG_S - 3
    assert A.indptr[c + 1] - A.indptr[c] >= 2
    idx[A.indptr[c] + 1] = idx[A.indptr[c]]
    bad_big = _lib.CscView(A.data, idx, A.indptr, A.shape, 0.0, copied=True)
    for plan in ("pipe=0", "pipe=1", None):
        ctx.debug_set_plan(plan)
        try:
            with pytest.raises(_lib.IciktError, match=rf"code -1.*duplicate entry \(sum_duplicates\).*column {c}\b"):
                ctx.pairs(bad_big, perspective="global", want_counts=False)
        finally:
            ctx.debug_set_plan(None)
        still_computes()
    got = ctx.pairs(A, perspective="global", want_counts=True)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert same(g, r), k


# ---- the front ends ----------------------------------------------------------------------------------------------------------

def same_result(a, b, path=""):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            if k != "run_time":
                same_result(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            same_result(x, y, f"{path}[{k}]")
    elif hasattr(a, "to_numpy"):
        assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index), path
        for col in a.columns:
            same_result(a[col].to_numpy(), b[col].to_numpy(), f"{path}/{col}")
    elif isinstance(a, np.ndarray) and a.dtype.kind in "fiub":
        assert same(a, b), path
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and all(x == y for x, y in zip(a.ravel(), b.ravel())), path
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), path
    else:
        assert a == b, path


@pytest.mark.parametrize("make", ["csc_matrix", "csr_matrix", "csc_array"])
def test_front_ends_on_a_sparse_matrix(hip_ctx, make):
    import icikendalltau_amd as pkg
    from tests.oracle_engine import OracleEngine
    M = count_like()
    A = getattr(sp, make)(M)
    D = A.toarray()
    S = M.shape[1]
    names = [f"s{j}" for j in range(S)]
    classes = ["a", "b", "a", "b", "a", "b", "a"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = pkg.ici_kendalltau(A, colnames=names)
        same_result(got, pkg.ici_kendalltau(D, colnames=names), "ici_kendalltau")
        cpu = pkg.ici_kendalltau(D, colnames=names, engine=OracleEngine())
        for key in ("cor", "raw", "pvalue", "taumax", "completeness"):
            g, r = np.asarray(got[key], dtype=np.float64), np.asarray(cpu[key], dtype=np.float64)
            assert np.array_equal(np.isnan(g), np.isnan(r)), key
            assert np.all(np.abs(g - r)[~np.isnan(g)] <= 1e-10), (key, np.nanmax(np.abs(g - r)))
        assert np.array_equal(np.asarray(got["keep"]), np.asarray(cpu["keep"]))
        for label, call in (
                ("pairwise_completeness", lambda X: pkg.pairwise_completeness(X, colnames=names)),
                ("test_left_censorship", lambda X: pkg.test_left_censorship(X, sample_classes=classes)),
                ("calculate_matrix_medians", lambda X: pkg.calculate_matrix_medians(X, na_rm=True)),
                ("rank_order_data", lambda X: pkg.rank_order_data(X, sample_classes=classes, colnames=names))):
            same_result(call(A), call(D), label)


def test_transposed_csr_goes_in_without_a_copy(hip_ctx):
    import icikendalltau_amd as pkg
    M = count_like()
    cells_by_genes = sp.csr_matrix(M.T)
    A = cells_by_genes.T
    v = _lib.csc_view(A)
    assert v.copied is False and np.shares_memory(v.data, cells_by_genes.data)
    names = [f"s{j}" for j in range(M.shape[1])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        same_result(pkg.ici_kendalltau(A, colnames=names), pkg.ici_kendalltau(M, colnames=names), "transposed CSR")
