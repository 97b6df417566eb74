"""_lib.csc_view and the front ends' sparse branches, without a GPU: which inputs keep their arrays, which are cast, how
`fill` travels, a duck-typed object without scipy, and a sparse matrix on the CPU engine."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib

sp = pytest.importorskip("scipy.sparse")

NA_REAL_BITS = 0x7FF00000000007A2


def count_matrix(dtype=np.float32, n=300, S=7, seed=5):
    rng = np.random.default_rng(seed)
    M = rng.integers(1, 31, size=(n, S)).astype(np.float64)
    M[rng.random((n, S)) < 0.6] = 0.0
    return M.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32, np.int64])
@pytest.mark.parametrize("make", ["csc_matrix", "csc_array"])
def test_supported_types_are_read_where_they_lie(dtype, make):
    A = getattr(sp, make)(count_matrix(dtype))
    v = _lib.csc_view(A)
    assert v.copied is False and v.shape == (300, 7)
    assert np.shares_memory(v.data, A.data) and np.shares_memory(v.indices, A.indices)
    assert np.shares_memory(v.indptr, A.indptr)
    s = v.struct()
    assert (s.values, s.indices, s.indptr) == (A.data.ctypes.data, A.indices.ctypes.data, A.indptr.ctypes.data)
    assert s.dtype == _lib.DTYPES[np.dtype(dtype)] and s.index_type == _lib.INDEX_TYPES[A.indices.dtype]
    assert np.array_equal(v.toarray(), A.toarray().astype(np.float64))


def test_int64_indices_are_read_where_they_lie():
    A = sp.csc_matrix(count_matrix())
    A.indices = A.indices.astype(np.int64)
    A.indptr = A.indptr.astype(np.int64)
    v = _lib.csc_view(A)
    assert v.copied is False and v.struct().index_type == _lib.INDEX_I64
    assert np.shares_memory(v.indices, A.indices)


def test_transposed_csr_is_csc_without_a_copy():
    cells_by_genes = sp.csr_matrix(count_matrix().T)          # AnnData's X
    A = cells_by_genes.T
    v = _lib.csc_view(A)
    assert v.copied is False and v.shape == (300, 7)
    assert np.shares_memory(v.data, cells_by_genes.data) and np.shares_memory(v.indices, cells_by_genes.indices)


@pytest.mark.parametrize("dtype,to", [(np.float16, np.float32), (np.uint8, np.int32), (np.uint32, np.int64),
                                      (np.bool_, np.int32)])
def test_other_value_types_are_cast(dtype, to):
    M = count_matrix(np.float64)
    A = sp.csc_matrix(M)
    A.data = A.data.astype(dtype)                             # (scipy's constructors refuse float16; the arrays do not)
    v = _lib.csc_view(A)
    assert v.copied is True and v.data.dtype == to
    assert np.array_equal(v.toarray(), M.astype(dtype).astype(np.float64))
    assert np.shares_memory(v.indices, A.indices)             # (only what needs a cast is cast)


def test_mixed_index_widths_are_cast_to_int64():
    A = sp.csc_matrix(count_matrix())
    A.indptr = A.indptr.astype(np.int64)
    assert A.indices.dtype == np.int32
    v = _lib.csc_view(A)
    assert v.copied is True and v.indices.dtype == np.int64 and v.indptr.dtype == np.int64
    assert np.array_equal(v.toarray(), A.toarray().astype(np.float64))


@pytest.mark.parametrize("make", ["csr_matrix", "coo_matrix"])
def test_other_formats_go_through_tocsc(make):
    M = count_matrix()
    A = getattr(sp, make)(M)
    v = _lib.csc_view(A)
    assert v.copied is True and v.format == "csc"
    assert np.array_equal(v.toarray(), M.astype(np.float64))


@pytest.mark.parametrize("bits", [0x0000000000000000, 0x8000000000000000, NA_REAL_BITS, 0x401E000000000000])
def test_fill_travels_bit_for_bit(bits):
    fill = np.array([bits], dtype=np.uint64).view(np.float64)[0]
    v = _lib.csc_view(sp.csc_matrix(count_matrix()), fill=fill)
    s = v.struct()
    raw = bytes((_lib.ctypes.c_char * 8).from_address(_lib.ctypes.addressof(s) + _lib.CscInput.fill.offset))
    assert raw == np.array([bits], dtype=np.uint64).tobytes()
    D = v.toarray()
    absent = sp.csc_matrix(count_matrix()).toarray() == 0
    assert np.all(D.view(np.uint64)[absent] == bits)
    again = _lib.csc_view(v)                                   # a view passes through with its fill
    assert again.fill.view(np.uint64)[0] == bits


class Duck:
    """What csc_view needs, and nothing of scipy's."""
    format = "csc"

    def __init__(self, M):
        n, S = M.shape
        self.shape = (n, S)
        cols = [np.flatnonzero(M[:, j]) for j in range(S)]
        self.indptr = np.concatenate(([0], np.cumsum([c.size for c in cols]))).astype(np.int32)
        self.indices = np.concatenate(cols).astype(np.int32)
        self.data = np.concatenate([M[c, j] for j, c in enumerate(cols)]).astype(M.dtype)


def test_a_duck_typed_object_without_scipy():
    M = count_matrix(np.int32)
    d = Duck(M)
    assert _lib.is_sparse(d) and not _lib.is_sparse(M) and not _lib.is_sparse([[1, 2]])
    v = _lib.csc_view(d)
    assert v.copied is False and np.shares_memory(v.data, d.data)
    assert np.array_equal(v.toarray(), M.astype(np.float64))
    d.format = "csr"                                          # no tocsc(): nothing csc_view could do with it
    assert not _lib.is_sparse(d)
    with pytest.raises(TypeError):
        _lib.csc_view(d)


def test_malformed_shapes_are_refused_on_the_host():
    A = sp.csc_matrix(count_matrix())
    d = Duck(count_matrix(np.int32))
    d.indptr = d.indptr[:-1]
    with pytest.raises(ValueError, match="indptr"):
        _lib.csc_view(d)
    with pytest.raises(TypeError):
        _lib.csc_view(A.toarray())


def same_result(a, b, path=""):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            if k != "run_time":
                same_result(a[k], b[k], f"{path}/{k}")
    elif hasattr(a, "to_numpy"):
        assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index), path
        for col in a.columns:
            same_result(a[col].to_numpy(), b[col].to_numpy(), f"{path}/{col}")
    elif isinstance(a, np.ndarray) and a.dtype.kind in "fiub":
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), path
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and all(x == y for x, y in zip(a.ravel(), b.ravel())), path
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            same_result(x, y, f"{path}[{k}]")
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), path
    else:
        assert a == b, path


@pytest.mark.parametrize("make", ["csc_matrix", "csr_matrix", "csc_array"])
def test_front_ends_on_the_cpu_engine_equal_the_dense_call(make):
    import icikendalltau_amd as pkg
    from tests.oracle_engine import OracleEngine
    M = count_matrix(np.float32, n=120, S=6)
    A = getattr(sp, make)(M)
    names = [f"s{j}" for j in range(M.shape[1])]
    classes = ["a", "b"] * 3
    eng = OracleEngine()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for label, call in (
                ("ici_kendalltau", lambda X: pkg.ici_kendalltau(X, colnames=names, engine=eng)),
                ("ici_kendalltau frame", lambda X: pkg.ici_kendalltau(X, colnames=names, engine=eng, return_matrix=False)),
                ("pairwise_completeness", lambda X: pkg.pairwise_completeness(X, colnames=names, engine=eng)),
                ("test_left_censorship", lambda X: pkg.test_left_censorship(X, sample_classes=classes, engine=eng)),
                ("calculate_matrix_medians", lambda X: pkg.calculate_matrix_medians(X, na_rm=True, engine=eng)),
                ("calculate_matrix_medians rows", lambda X: pkg.calculate_matrix_medians(X, use="row", engine=eng)),
                ("rank_order_data", lambda X: pkg.rank_order_data(X, sample_classes=classes, colnames=names, engine=eng)),
                ("kt_fast", lambda X: pkg.kt_fast(X, colnames=names, engine=eng)),
                ("cor_fast", lambda X: pkg.cor_fast(X, colnames=names, engine=eng))):
            same_result(call(A), call(M), label)


def test_front_ends_check_a_sparse_matrix_as_they_check_a_dense_one():
    import icikendalltau_amd as pkg
    from tests.oracle_engine import OracleEngine
    A = sp.csc_matrix(count_matrix(np.float32, n=40, S=4))
    with pytest.raises(ValueError, match="Colnames"):
        pkg.ici_kendalltau(A, engine=OracleEngine())
    with pytest.raises(ValueError, match="colnames"):
        pkg.ici_kendalltau(A, colnames=["a", "b"], engine=OracleEngine())
