"""ctypes binding of the C ABI in include/icikt.h (libicikt_hip.so, built in-tree by build()).

There is no CPU implementation behind this module: if the shared library is missing, or no HIP
device is usable, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.environ.get("ICIKT_LIB") or os.path.join(_PKG, "libicikt_hip.so")  # ICIKT_LIB: A/B of builds (tools)
SOURCES = [os.path.join(_PKG, "csrc", f) for f in ("icikt_kernels.hip", "icikt_prepass.hip", "icikt_epilogue.hip",
                                                       "icikt_capi.cpp", "icikt_pipeline.cpp", "icikt_capi_cor.cpp",
                                                       "icikt_capi_diag.cpp",
                                                       "icikt_multi.cpp", "icikt_transfer.cpp", "icikt_cor.hip", "icikt_topk.hip",
                                                       "icikt_capi_topk.cpp", "icikt_edges.hip", "icikt_capi_edges.cpp",
                                                       "icikt_diag.hip", "icikt_ingest.hip", "icikt_sparse.hip",
                                                       "icikt_medians.hip", "icikt_capi_medians.cpp", "icikt_capi_select.cpp",
                                                       "icikt_quantiles.hip", "icikt_capi_quantiles.cpp",
                                                       "icikt_classmat.hip", "icikt_capi_classmat.cpp",
                                                       "icikt_padjust.hip", "icikt_capi_padjust.cpp",
                                                       "icikt_mst.hip", "icikt_capi_mst.cpp",
                                                       "icikt_hclust.hip", "icikt_capi_hclust.cpp",
                                                       "icikt_anosim.hip", "icikt_capi_anosim.cpp",
                                                       "icikt_permanova.hip", "icikt_capi_permanova.cpp",
                                                       "icikt_permdisp.hip", "icikt_capi_permdisp.cpp",
                                                       "icikt_pcoa.hip", "icikt_capi_pcoa.cpp",
                                                       "icikt_mantel.hip", "icikt_capi_mantel.cpp",
                                                       "icikt_cross.hip", "icikt_capi_cross.cpp")]
HEADERS = [os.path.join(_ROOT, "include", "icikt.h"), os.path.join(_PKG, "csrc", "icikt_device.h"),
           os.path.join(_PKG, "csrc", "icikt_wave.h"), os.path.join(_PKG, "csrc", "icikt_host.h"),
           os.path.join(_PKG, "csrc", "icikt_transfer.h"), os.path.join(_PKG, "csrc", "icikt_colsort.h"),
           os.path.join(_PKG, "csrc", "icikt_blocks.h"), os.path.join(_PKG, "csrc", "icikt_select.h"),
           os.path.join(_PKG, "csrc", "icikt_keys.h"), os.path.join(_PKG, "csrc", "icikt_k0plan.h"),
           os.path.join(_PKG, "csrc", "icikt_k1plan.h"), os.path.join(_PKG, "csrc", "icikt_fixed.h"),
           os.path.join(_PKG, "csrc", "icikt_labels.h"), os.path.join(_PKG, "csrc", "icikt_ritz.h"),
           os.path.join(_PKG, "csrc", "icikt_mantel.h")]

# include/icikt.h
SUCCESS = 0
E_NO_DEVICE = -6
PERSPECTIVE = {"local": 0, "global": 1}
ALTERNATIVE = {"two.sided": 0, "less": 1, "greater": 2}
ALT_OTHER = 3
FLAG_EXACT_INT64 = 1
FLAG_TIMING = 2
FLAG_REUSE_COUNTS = 4
FLAG_BALANCE_COST = 16  # multi-device entries: pair blocks of equal cost (the streamed columns' tie structure) instead of equal length
FLAG_HOST_PINNED = 8     # the caller has page-locked the matrix and the result arrays of the call (pinned_empty)
CNT_FIELDS = ("n", "missing", "dis", "ntie", "xtie", "ytie", "x0", "x1", "y0", "y1", "tot")
K_PREPARE, K_PAIRS, K_EPILOGUE = 0, 1, 2
TOPK_MAX = 256                # ICIKT_TOPK_MAX: partners per sample of icikt_topk_*
TOPK_MAX_SAMPLES = 65535      # ICIKT_TOPK_MAX_SAMPLES
QUANTILE_MAX_PROBS = 32       # ICIKT_QUANTILE_MAX_PROBS: probabilities per call of icikt_quantiles_*
HIST_MAX_BINS = 1024          # ICIKT_HIST_MAX_BINS
ADJUST = {"bonferroni": 0, "holm": 1, "hochberg": 2, "BH": 3}   # ICIKT_ADJUST_*: R's p.adjust methods of icikt_padjust_*
ADJUST_MAX_ALPHA = 16         # ICIKT_ADJUST_MAX_ALPHA: alphas per call of icikt_padjust_*
HCLUST = {"complete": 0, "average": 1, "single": 2}   # ICIKT_HCLUST_*: linkage methods of icikt_hclust_*
ANOSIM_MAX_PERM = 1000000     # ICIKT_ANOSIM_MAX_PERM: labellings per call of icikt_anosim_* beside the observed one
PERMANOVA_MAX_CELLS = 1 << 26  # ICIKT_PERMANOVA_MAX_CELLS: (1 + n_perm) n_class of icikt_permanova_*
PERMDISP_MAX_CELLS = 1 << 26   # ICIKT_PERMDISP_MAX_CELLS: n_samp n_class of icikt_permdisp_*
MANTEL_MAX_PERM = 1000000      # ICIKT_MANTEL_MAX_PERM: permutations per call of icikt_mantel_*
MANTEL = {"pearson": 0, "spearman": 1}   # ICIKT_MANTEL_*: how icikt_mantel_* turns the two vectors into integers
PCOA_MAX_K = 64                # ICIKT_PCOA_MAX_K: eigenpairs per call of icikt_pcoa_*
PCOA_MAX_BASIS = 512           # ICIKT_PCOA_MAX_BASIS: basis columns of icikt_pcoa_*
MASK_VALS = 32                # distinct finite global_na values of the device-side exclusion rule (icikt_device.h)
MAX_FEATURES = 65535          # the tuned kernels
MAX_FEATURES_WIDE = 262144    # the plain 32-bit path (exact integer arithmetic)
PREP_ARRAYS = 5  # order, rec, hirow, meta (bitsets + stats per column), tgroups
PREP_EXCHANGE = (0, 3)  # order and meta: the rest is rebuilt by expand_cols_dev()

METHOD = {"pearson": 0, "spearman": 1}   # ICIKT_METHOD_*
COR_OK, COR_SHORT, COR_NA, COR_TIES = range(4)   # ICIKT_COR_*: per-pair reasons of icikt_cor_pairs_f64

REASON_OK, REASON_ALL_MISSING, REASON_SHORT, REASON_SINGLE_UNIQUE, REASON_TIES_EQ_TOTAL = range(5)
REASON_WARNINGS = {
    REASON_SHORT: "Warning: The vectors only have a single value, NA returned!",  # src/kendallc.cpp:225
    REASON_SINGLE_UNIQUE: "Warning: Either 'X' or 'Y' have only a single unique value, NA returned!",  # :238
    REASON_TIES_EQ_TOTAL: "Warning: Ties equal the total, NA returned!",  # :292
}

EXPORTS = (
    "icikt_version", "icikt_device_count", "icikt_ctx_create", "icikt_ctx_destroy", "icikt_last_error",
    "icikt_ctx_set_stream", "icikt_ctx_use_own_stream", "icikt_sync", "icikt_prepare_dev", "icikt_prepare_cols_dev", "icikt_prepare_cols_f64", "icikt_prep_arrays", "icikt_expand_cols_dev", "icikt_set_pairs", "icikt_set_pairs_combn",
    "icikt_num_pairs", "icikt_run_dev", "icikt_kernel_ms", "icikt_reset_timers", "icikt_pairs_f64",
    "icikt_pair_f64", "icikt_pairs_complete_f64", "icikt_missingness_f64", "icikt_selftest", "icikt_debug_set_plan",
    "icikt_multi_create", "icikt_multi_destroy", "icikt_multi_last_error", "icikt_multi_n_gpu", "icikt_multi_uses_rccl",
    "icikt_pairs_multi_f64", "icikt_multi_phase_ms", "icikt_multi_debug_set_plan",
    "icikt_matrix_f64", "icikt_matrix_multi_f64", "icikt_multi_rank_phase_ms", "icikt_multi_ranks_used",
    "icikt_debug_step_stats", "icikt_multi_comm_ranks", "icikt_multi_block_bounds", "icikt_cost_blocks",
    "icikt_cor_pairs_f64", "icikt_col_medians_f64", "icikt_censor_counts_f64", "icikt_rank_order_f64",
    "icikt_pairs_in", "icikt_matrix_in", "icikt_pairs_complete_in", "icikt_missingness_in", "icikt_cor_pairs_in",
    "icikt_col_medians_in", "icikt_censor_counts_in", "icikt_rank_order_in", "icikt_convert_dev",
    "icikt_pairs_csc", "icikt_matrix_csc", "icikt_missingness_csc", "icikt_col_medians_csc", "icikt_censor_counts_csc",
    "icikt_rank_order_csc", "icikt_scatter_csc_dev",
    "icikt_topk_f64", "icikt_topk_in", "icikt_topk_csc",
    "icikt_edges_f64", "icikt_edges_in", "icikt_edges_csc",
    "icikt_class_medians_f64", "icikt_class_medians_in", "icikt_class_medians_csc",
    "icikt_quantiles_f64", "icikt_quantiles_in", "icikt_quantiles_csc",
    "icikt_class_matrix_f64", "icikt_class_matrix_in", "icikt_class_matrix_csc",
    "icikt_padjust_f64", "icikt_padjust_in", "icikt_padjust_csc",
    "icikt_mst_f64", "icikt_mst_in", "icikt_mst_csc",
    "icikt_hclust_f64", "icikt_hclust_in", "icikt_hclust_csc",
    "icikt_anosim_f64", "icikt_anosim_in", "icikt_anosim_csc",
    "icikt_permanova_f64", "icikt_permanova_in", "icikt_permanova_csc",
    "icikt_permdisp_f64", "icikt_permdisp_in", "icikt_permdisp_csc",
    "icikt_pcoa_f64", "icikt_pcoa_in", "icikt_pcoa_csc", "icikt_pcoa_apply_dev",
    "icikt_mantel_f64", "icikt_mantel_in", "icikt_mantel_csc",
    "icikt_cross_f64", "icikt_cross_in",
    "icikt_ref_prepare_f64", "icikt_ref_prepare_in", "icikt_ref_cross_f64", "icikt_ref_cross_in", "icikt_ref_info",
)

# icikt_input: the caller's matrix as a typed, strided view (ICIKT_DTYPE_*, ICIKT_ORDER_*)
DTYPE_F64, DTYPE_F32, DTYPE_I32, DTYPE_I64 = range(4)
ORDER_COL, ORDER_ROW = 0, 1
DTYPES = {np.dtype(np.float64): DTYPE_F64, np.dtype(np.float32): DTYPE_F32, np.dtype(np.int32): DTYPE_I32,
          np.dtype(np.int64): DTYPE_I64}


class EdgeRule(ctypes.Structure):
    """icikt_edge_rule (include/icikt.h): a NaN bound is no bound."""
    _fields_ = [("min_raw", ctypes.c_double), ("max_pvalue", ctypes.c_double), ("min_completeness", ctypes.c_double),
                ("absolute", ctypes.c_int)]


def edge_rule(min_raw=None, max_pvalue=None, min_completeness=None, absolute=False) -> EdgeRule:
    """The icikt_edge_rule of the three bounds (None: no bound)."""
    nan = float("nan")
    return EdgeRule(nan if min_raw is None else float(min_raw), nan if max_pvalue is None else float(max_pvalue),
                    nan if min_completeness is None else float(min_completeness), int(bool(absolute)))


class InputView(ctypes.Structure):
    """icikt_input (include/icikt.h)."""
    _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int), ("order", ctypes.c_int), ("ld", ctypes.c_int64)]


def input_view(X):
    """(array, dtype code, order, ld, copied): how the *_in entries read X where it lies.  No copy is made of a 2-D,
    aligned, native-endian ndarray of float64, float32, int32 or int64 whose strides are (itemsize, k * itemsize) with
    k >= n_feat (ORDER_COL, ld = k) or (k * itemsize, itemsize) with k >= n_samp (ORDER_ROW, ld = k): contiguous arrays
    of either order and their slices X[:, a:b], X[a:b, :].  Everything else is copied to an F-ordered float64 array
    (copied = True), as every matrix was before the view existed."""
    if (isinstance(X, np.ndarray) and X.ndim == 2 and X.size > 0 and X.dtype in DTYPES and X.dtype.isnative
            and X.flags.aligned):
        n_feat, n_samp = X.shape
        it = X.dtype.itemsize
        s0, s1 = X.strides
        code = DTYPES[X.dtype]
        # (a dimension of extent 1 has a stride numpy never uses: such an array is read in the order the other
        #  stride fits, column-major first)
        if (s0 == it or n_feat == 1) and ((s1 > 0 and s1 % it == 0 and s1 // it >= n_feat) or n_samp == 1):
            return X, code, ORDER_COL, (n_feat if n_samp == 1 else s1 // it), False
        if (s1 == it or n_samp == 1) and ((s0 > 0 and s0 % it == 0 and s0 // it >= n_samp) or n_feat == 1):
            return X, code, ORDER_ROW, (n_samp if n_feat == 1 else s0 // it), False
    Xf = np.asfortranarray(X, dtype=np.float64)
    if Xf.ndim != 2:
        raise ValueError("X must be 2-D (features x samples)")
    return Xf, DTYPE_F64, ORDER_COL, max(Xf.shape[0], 1), True


def _view_arg(X, flags: int = 0):
    """(array kept alive, icikt_input by reference, n_feat, n_samp, flags): FLAG_HOST_PINNED speaks of the caller's
    memory, so it is cleared when the entry reads a copy of the library's own making.  A sparse matrix (is_sparse) gives
    its CscView and an icikt_csc_input instead: the *_csc entries take it where the *_in entries take the dense view."""
    if is_sparse(X):
        s = csc_view(X)
        return s, s.struct(), s.shape[0], s.shape[1], (flags & ~FLAG_HOST_PINNED) if s.copied else flags
    a, code, order, ld, copied = input_view(X)
    v = InputView(a.ctypes.data, code, order, ld)
    return a, v, a.shape[0], a.shape[1], (flags & ~FLAG_HOST_PINNED) if copied else flags


# icikt_csc_input: the caller's matrix in compressed-sparse-column form (ICIKT_INDEX_*)
INDEX_I32, INDEX_I64 = 0, 1
INDEX_TYPES = {np.dtype(np.int32): INDEX_I32, np.dtype(np.int64): INDEX_I64}


class CscInput(ctypes.Structure):
    """icikt_csc_input (include/icikt.h)."""
    _fields_ = [("values", ctypes.c_void_p), ("indices", ctypes.c_void_p), ("indptr", ctypes.c_void_p),
                ("dtype", ctypes.c_int), ("index_type", ctypes.c_int), ("fill", ctypes.c_double)]


class CscView:
    """A features x samples matrix in CSC form as the *_csc entries read it (csc_view builds it): data / indices /
    indptr as numpy arrays of supported types, shape, fill (a one-element float64 array: its 64 bits travel as they
    are), and copied: whether any of the three arrays is a copy csc_view made (a cast, or tocsc)."""

    def __init__(self, data, indices, indptr, shape, fill, copied):
        self.data, self.indices, self.indptr = data, indices, indptr
        self.shape = (int(shape[0]), int(shape[1]))
        self.fill = np.array([fill], dtype=np.float64) if not isinstance(fill, np.ndarray) else fill
        self.copied = bool(copied)
        self.format = "csc"

    def struct(self):
        """The icikt_csc_input of this view (the view must outlive the call that gets it)."""
        v = CscInput(self.data.ctypes.data if self.data.size else None,
                     self.indices.ctypes.data if self.indices.size else None, self.indptr.ctypes.data,
                     DTYPES[self.data.dtype], INDEX_TYPES[self.indices.dtype], 0.0)
        ctypes.memmove(ctypes.addressof(v) + CscInput.fill.offset, self.fill.ctypes.data, 8)   # (the bits, whatever they are)
        return v

    def toarray(self):
        """The dense column-major float64 matrix the view stands for (the definition in include/icikt.h; duplicates:
        the last one wins here, the library refuses them)."""
        n, S = self.shape
        M = np.empty((n, S), dtype=np.float64, order="F")
        M.view(np.uint64)[...] = self.fill.view(np.uint64)[0]
        cols = np.repeat(np.arange(S), np.diff(self.indptr[:S + 1]))
        lo, hi = int(self.indptr[0]), int(self.indptr[S])
        M[self.indices[lo:hi], cols] = self.data[lo:hi]
        return M


def is_sparse(A) -> bool:
    """A CscView, or anything that looks like a scipy.sparse matrix / array (scipy itself is never imported here): a
    `format` string and a 2-D `shape`, and either the CSC arrays or a `tocsc` method."""
    if isinstance(A, CscView):
        return True
    if isinstance(A, np.ndarray) or not isinstance(getattr(A, "format", None), str):
        return False
    if len(getattr(A, "shape", ())) != 2:
        return False
    return hasattr(A, "tocsc") or (A.format == "csc" and all(hasattr(A, k) for k in ("data", "indices", "indptr")))


def csc_view(A, fill=0.0) -> CscView:
    """How the *_csc entries read a sparse matrix A (features x samples): duck-typed on .format == "csc", .data,
    .indices, .indptr and .shape, so scipy stays optional.  The three arrays stay where they lie (copied = False) when
    data is float64, float32, int32 or int64 and indices / indptr share int32 or int64 -- which holds for
    scipy.sparse.csc_matrix / csc_array and for the transpose of a CSR matrix (cells x genes -> features x samples).
    Anything else is cast, O(nnz) on the host: float16 -> float32, other floats -> float64, bool and integers of up to
    32 bits -> int32 (uint32 -> int64), uint64 -> float64; mixed or other index types -> int64.  Any other sparse format
    (csr, coo, ...) goes through A.tocsc(), also O(nnz) on the host.  fill: the value of every cell without an entry
    (0.0: scipy's toarray), carried bit for bit."""
    if isinstance(A, CscView):
        if isinstance(fill, (int, float)) and fill == 0.0 and not np.signbit(fill):
            return A
        return CscView(A.data, A.indices, A.indptr, A.shape, np.array([fill], dtype=np.float64), A.copied)
    if not is_sparse(A):
        raise TypeError("csc_view needs a sparse matrix (an object with .format, .shape and the CSC arrays or .tocsc())")
    copied = False
    if A.format != "csc":
        A = A.tocsc()
        copied = True
    data, indices, indptr = np.asarray(A.data), np.asarray(A.indices), np.asarray(A.indptr)
    n_feat, n_samp = (int(v) for v in A.shape)
    if data.ndim != 1 or indices.ndim != 1 or indptr.ndim != 1 or indptr.shape[0] != n_samp + 1:
        raise ValueError("a CSC matrix needs 1-D data / indices and n_samp + 1 column offsets in indptr")
    if indices.shape[0] < data.shape[0]:
        raise ValueError("a CSC matrix needs a row index for every stored value")

    def plain(a):
        return a.dtype.isnative and a.flags.c_contiguous and a.flags.aligned

    if not (data.dtype in DTYPES and plain(data)):
        k, size = data.dtype.kind, data.dtype.itemsize
        if k == "f":
            to = np.float32 if size <= 4 else np.float64
        elif k == "b" or (k == "i" and size <= 4) or (k == "u" and size < 4):
            to = np.int32
        elif k in "iu" and (k == "i" or size == 4):
            to = np.int64
        elif k == "u":
            to = np.float64
        else:
            raise TypeError("the values of a sparse matrix must be of a numeric type")
        data = np.ascontiguousarray(data, dtype=to)
        copied = True
    if not (indices.dtype == indptr.dtype and indices.dtype in INDEX_TYPES and plain(indices) and plain(indptr)):
        if indices.dtype.kind not in "iu" or indptr.dtype.kind not in "iu":
            raise TypeError("indices and indptr of a sparse matrix must be integers")
        narrow = indices.dtype.itemsize <= 4 and indptr.dtype.itemsize <= 4 and \
            indices.dtype != np.uint32 and indptr.dtype != np.uint32
        to = np.int32 if narrow else np.int64
        indices = np.ascontiguousarray(indices, dtype=to)
        indptr = np.ascontiguousarray(indptr, dtype=to)
        copied = True
    f = np.array([fill], dtype=np.float64) if not isinstance(fill, np.ndarray) else np.ascontiguousarray(fill, dtype=np.float64).reshape(1)
    return CscView(data, indices, indptr, (n_feat, n_samp), f, copied)



class IciktError(RuntimeError):
    pass


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > t for p in SOURCES + HEADERS)


def build(force: bool = False, verbose: bool = False, extra_flags=(), out: str | None = None) -> str:
    """Compile the HIP kernels + C ABI for gfx950 into icikendalltau_amd/libicikt_hip.so (or, for the development
    tools, a variant build with extra_flags into `out`: loaded through ICIKT_LIB)."""
    if out is None and not force and not needs_build():
        return LIB_PATH
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared", *extra_flags,
           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_PKG, "csrc"),
           "-o", out or LIB_PATH] + SOURCES + ["-L", os.path.join(rocm, "lib"), "-lrccl", "-pthread"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise IciktError("hipcc failed:\n" + res.stdout + res.stderr)
    if verbose:
        print(" ".join(cmd))
    return out or LIB_PATH


_lib = None


def lib():
    """Load the shared library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1.
    # Importing torch FIRST lets the dynamic linker satisfy this library's NEEDED sonames with torch's
    # copies; the other order loads /opt/rocm's runtime beside torch's and the second one finds no device.
    if os.environ.get("ICIKT_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(LIB_PATH):
        raise IciktError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc); "
            "icikendalltau_amd has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    c_int, c_i64, c_u32, c_vp = ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p
    L.icikt_version.restype = c_int
    L.icikt_device_count.argtypes = [ctypes.POINTER(c_int)]
    L.icikt_ctx_create.argtypes = [c_int, ctypes.POINTER(c_vp)]
    L.icikt_ctx_destroy.argtypes = [c_vp]
    L.icikt_ctx_destroy.restype = None
    L.icikt_last_error.argtypes = [c_vp]
    L.icikt_last_error.restype = ctypes.c_char_p
    L.icikt_ctx_set_stream.argtypes = [c_vp, c_vp]
    L.icikt_ctx_use_own_stream.argtypes = [c_vp]
    L.icikt_sync.argtypes = [c_vp]
    L.icikt_prepare_dev.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_u32]
    L.icikt_prepare_cols_dev.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_u32]
    L.icikt_prepare_cols_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_u32]
    L.icikt_prep_arrays.argtypes = [c_vp, ctypes.POINTER(c_vp), ctypes.POINTER(c_i64)]
    L.icikt_expand_cols_dev.argtypes = [c_vp, c_i64, c_i64, c_u32]
    L.icikt_set_pairs.argtypes = [c_vp, c_vp, c_vp, c_i64]
    L.icikt_set_pairs_combn.argtypes = [c_vp, c_i64, c_i64, c_i64]
    L.icikt_num_pairs.argtypes = [c_vp]
    L.icikt_num_pairs.restype = c_i64
    L.icikt_run_dev.argtypes = [c_vp, c_int, c_int, c_int, c_u32, c_vp, c_vp, c_vp]
    L.icikt_kernel_ms.argtypes = [c_vp, c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_i64)]
    L.icikt_reset_timers.argtypes = [c_vp]
    L.icikt_pairs_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_i64, c_int, c_int, c_int, c_u32,
                                  c_vp, c_vp, c_vp]
    L.icikt_pairs_complete_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_i64, c_int, c_int, c_u32,
                                           c_vp, c_vp, c_vp]
    L.icikt_pair_f64.argtypes = [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_int, c_u32, c_vp, c_vp, c_vp]
    L.icikt_missingness_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp]
    L.icikt_cor_pairs_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_i64, c_int, c_int, c_int, c_int,
                                      c_u32, c_vp, c_vp]
    L.icikt_col_medians_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_u32, c_vp]
    L.icikt_censor_counts_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_vp, c_int, c_u32, c_vp, c_vp,
                                          c_vp, c_vp]
    L.icikt_rank_order_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_vp, c_i64, c_u32, c_vp, c_vp,
                                       c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_selftest.argtypes = [c_vp]
    L.icikt_debug_set_plan.argtypes = [c_vp, ctypes.c_char_p]
    L.icikt_multi_create.argtypes = [ctypes.POINTER(c_int), c_int, c_int, ctypes.POINTER(c_vp)]
    L.icikt_multi_destroy.argtypes = [c_vp]
    L.icikt_multi_destroy.restype = None
    L.icikt_multi_last_error.argtypes = [c_vp]
    L.icikt_multi_last_error.restype = ctypes.c_char_p
    L.icikt_multi_n_gpu.argtypes = [c_vp]
    L.icikt_multi_uses_rccl.argtypes = [c_vp]
    L.icikt_multi_comm_ranks.argtypes = [c_vp]
    L.icikt_multi_block_bounds.argtypes = [c_vp, ctypes.POINTER(c_i64)]
    L.icikt_cost_blocks.argtypes = [c_vp, c_i64, c_vp, c_i64, c_int, c_i64, c_vp]
    L.icikt_pairs_multi_f64.argtypes = L.icikt_pairs_f64.argtypes
    L.icikt_multi_phase_ms.argtypes = [c_vp, ctypes.POINTER(ctypes.c_double)]
    L.icikt_multi_debug_set_plan.argtypes = [c_vp, ctypes.c_char_p]
    L.icikt_matrix_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_vp, c_vp, c_i64, c_int, c_int, c_int,
                                   c_u32, c_int, c_int, c_vp, c_vp, c_vp]
    L.icikt_matrix_multi_f64.argtypes = L.icikt_matrix_f64.argtypes
    L.icikt_topk_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_int, c_u32, c_int,
                                 c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_edges_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, ctypes.POINTER(EdgeRule), c_int, c_int,
                                  c_int, c_u32, c_int, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_class_medians_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int,
                                          c_u32, c_int, c_vp, c_vp, c_vp, c_vp]
    L.icikt_class_matrix_f64.argtypes = L.icikt_class_medians_f64.argtypes
    L.icikt_quantiles_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int,
                                      c_u32, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                      c_vp]
    L.icikt_padjust_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_u32, c_int, c_vp,
                                    c_int, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_mst_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_u32, c_int,
                                ctypes.c_double, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_hclust_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_u32, c_int, c_int,
                                   ctypes.c_double, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_anosim_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_u32, c_vp, c_int,
                                   c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_permanova_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_u32, c_vp,
                                      c_int, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_permdisp_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_u32, c_vp,
                                     c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_pcoa_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_u32, c_int,
                                 ctypes.c_double, c_int, c_vp] + [c_vp] * 13
    L.icikt_mantel_f64.argtypes = [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_u32, c_vp, c_int,
                                   c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.icikt_pcoa_apply_dev.argtypes = [c_vp, c_vp, c_vp, c_i64, c_int, c_vp]
    # (two matrices: the twins are spelled out)
    cross_tail = [c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_int, c_int, c_int, c_u32, c_int, c_vp, c_vp, c_vp, c_vp, c_vp,
                  c_vp]
    L.icikt_cross_f64.argtypes = [c_vp, c_vp, c_i64, c_vp, c_i64] + cross_tail
    L.icikt_cross_in.argtypes = [c_vp, ctypes.POINTER(InputView), ctypes.POINTER(InputView)] + cross_tail
    ref_prepare_tail = [c_i64, c_i64, c_i64, c_vp, c_int, c_u32]
    L.icikt_ref_prepare_f64.argtypes = [c_vp, c_vp, c_i64] + ref_prepare_tail
    L.icikt_ref_prepare_in.argtypes = [c_vp, ctypes.POINTER(InputView)] + ref_prepare_tail
    ref_cross_tail = [c_i64, c_i64, c_int, c_vp, c_int, c_int, c_int, c_int, c_u32, c_int] + [c_vp] * 8
    L.icikt_ref_cross_f64.argtypes = [c_vp, c_vp, c_i64] + ref_cross_tail
    L.icikt_ref_cross_in.argtypes = [c_vp, ctypes.POINTER(InputView)] + ref_cross_tail
    L.icikt_ref_info.argtypes = [c_vp, c_vp, c_vp, c_vp]
    L.icikt_multi_rank_phase_ms.argtypes = [c_vp, c_int, ctypes.POINTER(ctypes.c_double)]
    L.icikt_multi_ranks_used.argtypes = [c_vp]
    L.icikt_debug_step_stats.argtypes = [c_vp, c_vp, c_int]
    # the *_in twins: (ctx, const icikt_input*, n_feat, n_samp, ...) where the _f64 entry has (ctx, X, n_feat, n_samp, ld, ...)
    for nm in ("pairs", "matrix", "pairs_complete", "missingness", "cor_pairs", "col_medians", "censor_counts",
               "rank_order", "topk", "edges", "class_medians", "quantiles", "class_matrix", "padjust", "mst", "hclust", "anosim",
               "permanova", "permdisp", "pcoa", "mantel"):
        f64 = getattr(L, f"icikt_{nm}_f64").argtypes
        getattr(L, f"icikt_{nm}_in").argtypes = [c_vp, ctypes.POINTER(InputView), c_i64, c_i64] + list(f64[5:])
    L.icikt_convert_dev.argtypes = [c_vp, c_vp, c_int, c_int, c_i64, c_i64, c_i64, c_vp, c_i64]
    # the *_csc twins: (ctx, const icikt_csc_input*, n_feat, n_samp, ...)
    for nm in ("pairs", "matrix", "missingness", "col_medians", "censor_counts", "rank_order", "topk", "edges",
               "class_medians", "quantiles", "class_matrix", "padjust", "mst", "hclust", "anosim",
               "permanova", "permdisp", "pcoa", "mantel"):
        f64 = getattr(L, f"icikt_{nm}_f64").argtypes
        getattr(L, f"icikt_{nm}_csc").argtypes = [c_vp, ctypes.POINTER(CscInput), c_i64, c_i64] + list(f64[5:])
    L.icikt_scatter_csc_dev.argtypes = [c_vp, c_vp, c_vp, c_vp, c_int, c_int, ctypes.c_double, c_i64, c_i64, c_vp, c_i64]
    for name in EXPORTS:
        if getattr(L, name).restype is not None and name not in ("icikt_last_error", "icikt_num_pairs",
                                                                   "icikt_multi_last_error"):
            getattr(L, name).restype = c_int
    _lib = L
    return L


def device_count() -> int:
    n = ctypes.c_int(0)
    lib().icikt_device_count(ctypes.byref(n))
    return n.value


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def pinned_empty(shape, dtype=np.float64, order="C"):
    """A numpy array in PAGE-LOCKED host memory (hipHostMalloc through torch's pinned allocator; the array keeps the
    tensor alive).  Host entries called with FLAG_HOST_PINNED copy from / into such arrays directly."""
    import torch
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    n = int(np.prod(shape)) if shape else 1
    t = torch.empty(max(n, 1) * np.dtype(dtype).itemsize, dtype=torch.uint8, pin_memory=True)
    a = t.numpy()[:n * np.dtype(dtype).itemsize].view(dtype).reshape(shape, order=order)
    return a


def _matrix_call(fn, handle, chk, X, global_na, pi, pj, perspective, alternative, continuity, flags, scale_max,
                 diag_good, want_keep, view=False):
    """icikt_matrix_in (view) / icikt_matrix_f64 / icikt_matrix_multi_f64: (out5 [5, S, S], keep [S, n_feat] bool or
    None, reason_counts [5])."""
    if view:
        X, v, n_feat, n_samp, flags = _view_arg(X, flags)
        xargs = (ctypes.byref(v), n_feat, n_samp)
    else:
        if is_sparse(X):
            X = csc_view(X).toarray()
            flags &= ~FLAG_HOST_PINNED
        if not (isinstance(X, np.ndarray) and X.dtype == np.float64 and X.ndim == 2 and X.flags.f_contiguous):
            X = np.asfortranarray(X, dtype=np.float64)
            flags &= ~FLAG_HOST_PINNED   # (a pageable copy of this function's)
        n_feat, n_samp = X.shape
        xargs = (_ptr(X), n_feat, n_samp, max(n_feat, 0))
    gna = np.ascontiguousarray([] if global_na is None else np.atleast_1d(global_na), dtype=np.float64)
    if pi is None:
        pi_a = pj_a = None
        P = 0
    else:
        pi_a = np.ascontiguousarray(pi, dtype=np.int32)
        pj_a = np.ascontiguousarray(pj, dtype=np.int32)
        P = pi_a.shape[0]
    alloc = pinned_empty if (flags & FLAG_HOST_PINNED) else np.empty   # the result arrays are this function's: pinned when the call says so
    out5 = alloc((5, n_samp, n_samp), dtype=np.float64)
    keep = alloc((n_samp, n_feat), dtype=np.uint8) if want_keep else None
    rc5 = np.zeros(5, dtype=np.int64)
    alt = ALTERNATIVE.get(alternative, ALT_OTHER)
    chk(fn(handle, *xargs, _ptr(gna) if gna.size else None, int(gna.size), _ptr(pi_a),
           _ptr(pj_a), P, PERSPECTIVE[perspective], alt, int(bool(continuity)), flags, int(bool(scale_max)),
           int(bool(diag_good)), _ptr(out5), _ptr(keep), _ptr(rc5)), fn.__name__)
    return out5, (keep.view(np.bool_) if keep is not None else None), rc5


class _SelectCall:
    """What the fourteen selection entries (topk, cross, edges, class_medians, class_matrix, quantiles, padjust, mst, hclust,
    anosim, permanova, permdisp, pcoa, mantel) share around their own arguments.  An instance holds a resolved entry (what Context._entry returns; the
    array behind its arguments stays alive with it), n_samp and flags as that entry sees them, and alloc: the allocator
    of the result arrays that are pinned when the call says so.  Calling it makes the checked call fn(ctx, <X>,
    global_na, n_global_na, *before, perspective, alternative, continuity, flags[, scale_max], *after, max_taumax,
    reason_counts) and returns (max_taumax, reason_counts [5]); scale_max None: the entry has no such argument."""

    def __init__(self, ctx, entry):
        self.ctx = ctx
        self.fn, self.fname, self.xargs, _n_feat, self.n_samp, self.flags, self._keep = entry
        self.alloc = pinned_empty if (self.flags & FLAG_HOST_PINNED) else np.empty

    def tree_room(self):
        """The S - 1 slots of mst's edges and hclust's merges (the library refuses more samples before it writes)."""
        return max(self.n_samp - 1, 0) if self.n_samp <= TOPK_MAX_SAMPLES else 0

    def __call__(self, global_na, perspective, alternative, continuity, scale_max, before=(), after=()):
        gna = np.ascontiguousarray([] if global_na is None else np.atleast_1d(global_na), dtype=np.float64)
        persp = PERSPECTIVE.get(perspective, perspective if isinstance(perspective, int) else -1)
        scale = () if scale_max is None else (int(bool(scale_max)),)
        mx, rc5 = np.full(1, -np.inf), np.zeros(5, dtype=np.int64)
        self.ctx._chk(self.fn(self.ctx._h, *self.xargs, _ptr(gna) if gna.size else None, int(gna.size), *before, persp,
                              ALTERNATIVE.get(alternative, ALT_OTHER), int(bool(continuity)), self.flags, *scale, *after,
                              _ptr(mx), _ptr(rc5)), self.fname)
        return float(mx[0]), rc5


def _class_arg(cls, n_samp):
    """cls of class_medians, class_matrix, quantiles, anosim and permanova as the library takes it: None (one class), or
    a contiguous int32 class index per column."""
    if cls is None:
        return None
    cls_a = np.ascontiguousarray(cls, dtype=np.int32)
    if cls_a.shape != (n_samp,):
        raise ValueError("cls must give one class per column")
    return cls_a


def _labellings_arg(cls, n_class, perm_cls, n_samp):
    """cls, n_class and perm_cls of anosim and permanova as the library takes them, and the room their results need:
    (cls_a, n_class, perm_a, n_perm, room, n_lab) with room the classes and n_lab the labellings the library may write
    (it refuses what is past its limits before it writes: the arrays are then of one class, one labelling)."""
    cls_a = _class_arg(cls, n_samp)
    if cls_a is None:
        n_class = 1
    n_class = int(n_class)
    if perm_cls is None:
        perm_a, n_perm = None, 0
    else:
        perm_a = np.ascontiguousarray(perm_cls, dtype=np.int32)
        if perm_a.ndim != 2 or perm_a.shape[1] != n_samp:
            raise ValueError("perm_cls must be [n_perm, S]: one class per column in every row")
        n_perm = int(perm_a.shape[0])
    room = n_class if 1 <= n_class <= 65535 else 1
    n_lab = 1 + (n_perm if n_perm <= ANOSIM_MAX_PERM else 0)
    return cls_a, n_class, perm_a, n_perm, room, n_lab


def _limbs_to_ints(lo, hi):
    """hi 2^32 + lo of two int64 arrays of non-negative limbs (lo < 2^48) as an object array of Python ints.  While every
    hi is below 2^30 the sum fits 63 bits and is taken in int64: one conversion of the table instead of three passes of
    Python arithmetic over it."""
    if hi.size == 0 or (int(hi.max()) < (1 << 30) and int(lo.max()) < (1 << 48)):
        return ((hi << 32) + lo).astype(object)
    return hi.astype(object) * (1 << 32) + lo.astype(object)


class Context:
    """One HIP device + stream + workspaces (icikt_ctx)."""

    def __init__(self, device: int = 0):
        self._h = ctypes.c_void_p()
        rc = lib().icikt_ctx_create(int(device), ctypes.byref(self._h))
        if rc == E_NO_DEVICE:
            raise IciktError("no usable HIP device: icikendalltau_amd computes on an MI355X only (no CPU fallback)")
        if rc != SUCCESS:
            raise IciktError(f"icikt_ctx_create(device={device}) failed with code {rc}")
        self.device = int(device)
        self.f64_entries = False   # tests / tools: the host methods call the _f64 entries on an F-ordered float64 copy

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().icikt_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int, what: str):
        if rc != SUCCESS:
            msg = lib().icikt_last_error(self._h)
            raise IciktError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")

    # -- device-resident path --------------------------------------------------------------------
    def set_stream(self, hip_stream: int | None):
        """Run on an existing hipStream_t (0 / None = HIP's default stream, e.g. torch's default)."""
        self._chk(lib().icikt_ctx_set_stream(self._h, ctypes.c_void_p(hip_stream or 0)), "icikt_ctx_set_stream")

    def use_own_stream(self):
        self._chk(lib().icikt_ctx_use_own_stream(self._h), "icikt_ctx_use_own_stream")

    def sync(self):
        self._chk(lib().icikt_sync(self._h), "icikt_sync")

    def prepare_dev(self, d_ptr: int, n_feat: int, n_samp: int, ld: int, flags: int = 0):
        self._chk(lib().icikt_prepare_dev(self._h, ctypes.c_void_p(d_ptr), n_feat, n_samp, ld, flags),
                  "icikt_prepare_dev")

    def prepare_cols_dev(self, d_ptr: int, n_feat: int, n_samp: int, ld: int, col_begin: int, col_end: int,
                         alloc_cols: int, flags: int = 0):
        """Pre-pass over columns [col_begin, col_end) only (multi-rank: all-gather prep_arrays() afterwards)."""
        self._chk(lib().icikt_prepare_cols_dev(self._h, ctypes.c_void_p(d_ptr), n_feat, n_samp, ld, col_begin,
                                               col_end, alloc_cols, flags), "icikt_prepare_cols_dev")

    def prepare_cols(self, X, col_begin: int, col_end: int, alloc_cols: int, flags: int = 0):
        """Pre-pass over columns [col_begin, col_end) of a HOST matrix (F-ordered float64, NaN = missing): only
        those columns cross PCIe."""
        if not (isinstance(X, np.ndarray) and X.dtype == np.float64 and X.flags.f_contiguous and X.ndim == 2):
            raise ValueError("prepare_cols needs a Fortran-ordered float64 matrix")
        n_feat, n_samp = X.shape
        self._chk(lib().icikt_prepare_cols_f64(self._h, _ptr(X), n_feat, n_samp, max(n_feat, 0), col_begin, col_end,
                                               alloc_cols, flags), "icikt_prepare_cols_f64")

    def prep_arrays(self):
        """[(device pointer, bytes per column)] of the prepared-state arrays."""
        ptrs = (ctypes.c_void_p * PREP_ARRAYS)()
        bpc = (ctypes.c_int64 * PREP_ARRAYS)()
        self._chk(lib().icikt_prep_arrays(self._h, ptrs, bpc), "icikt_prep_arrays")
        return [(int(ptrs[i] or 0), int(bpc[i])) for i in range(PREP_ARRAYS)]

    def expand_cols_dev(self, col_begin: int, col_end: int, flags: int = 0):
        """Rebuild rec / hirow / girow / tgroups and the tie program with its step records of columns [col_begin, col_end)
        from their (received) order and gflag."""
        self._chk(lib().icikt_expand_cols_dev(self._h, col_begin, col_end, flags), "icikt_expand_cols_dev")

    def set_pairs(self, pi, pj):
        pi = np.ascontiguousarray(pi, dtype=np.int32)
        pj = np.ascontiguousarray(pj, dtype=np.int32)
        if pi.shape != pj.shape or pi.ndim != 1:
            raise ValueError("pi and pj must be 1-D arrays of the same length")
        self._chk(lib().icikt_set_pairs(self._h, _ptr(pi), _ptr(pj), pi.shape[0]), "icikt_set_pairs")

    def set_pairs_combn(self, n_samp: int, begin: int, end: int):
        self._chk(lib().icikt_set_pairs_combn(self._h, n_samp, begin, end), "icikt_set_pairs_combn")

    def num_pairs(self) -> int:
        return int(lib().icikt_num_pairs(self._h))

    def run_dev(self, perspective: int, alternative: int, continuity: bool, flags: int, d_out4: int,
                d_counts: int | None = None, d_reasons: int | None = None):
        self._chk(lib().icikt_run_dev(self._h, perspective, alternative, int(bool(continuity)), flags,
                                      ctypes.c_void_p(d_out4), ctypes.c_void_p(d_counts or 0),
                                      ctypes.c_void_p(d_reasons or 0)), "icikt_run_dev")

    def kernel_ms(self, kernel: int):
        ms = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        self._chk(lib().icikt_kernel_ms(self._h, kernel, ctypes.byref(ms), ctypes.byref(n)), "icikt_kernel_ms")
        return ms.value, n.value

    def reset_timers(self):
        self._chk(lib().icikt_reset_timers(self._h), "icikt_reset_timers")

    def selftest(self):
        self._chk(lib().icikt_selftest(self._h), "icikt_selftest")

    def step_stats(self, reset: bool = True):
        """Diagnostic builds only (-DICIKT_STEP_STATS): {kind: (steps, rows, wave cycles)} of the pair kernel."""
        buf = np.zeros(24, dtype=np.uint64)
        self._chk(lib().icikt_debug_step_stats(self._h, _ptr(buf), int(reset)), "icikt_debug_step_stats")
        kinds = ("hot_loop", "hot_in_main_or_solo", "mixed", "group_rest", "group_top_phaseA", "tail", "setup", "group_close_insert_rebuild")
        return {k: (int(buf[i]), int(buf[8 + i]), int(buf[16 + i])) for i, k in enumerate(kinds)}

    def debug_set_plan(self, spec: str | dict | None = None):
        """Test / experiment hook: override the pair kernel's launch plan ("np=1,pend=g,..." or a dict; None resets)."""
        if isinstance(spec, dict):
            spec = ",".join(f"{k}={v}" for k, v in spec.items() if v not in ("", None))
        self._chk(lib().icikt_debug_set_plan(self._h, (spec or "").encode()), "icikt_debug_set_plan")

    # -- host-buffer path ------------------------------------------------------------------------
    def _entry(self, name, X, flags=0, ld_floor=0):
        """(entry function, its name, the arguments that describe X, n_feat, n_samp, flags, the array to keep alive):
        icikt_<name>_in on input_view(X), read where it lies; with f64_entries icikt_<name>_f64 on an F-ordered
        float64 copy."""
        sparse = is_sparse(X)
        if self.f64_entries:
            Xf = csc_view(X).toarray() if sparse else np.asfortranarray(X, dtype=np.float64)
            if Xf.ndim != 2:
                raise ValueError("X must be 2-D (features x samples)")
            if Xf is not X:
                flags &= ~FLAG_HOST_PINNED
            n_feat, n_samp = Xf.shape
            fn = f"icikt_{name}_f64"
            return getattr(lib(), fn), fn, (_ptr(Xf), n_feat, n_samp, max(n_feat, ld_floor)), n_feat, n_samp, flags, Xf
        a, v, n_feat, n_samp, flags = _view_arg(X, flags)
        fn = f"icikt_{name}_csc" if sparse else f"icikt_{name}_in"
        if sparse and not hasattr(lib(), fn):
            raise IciktError(f"{name}: no entry for a sparse matrix (densify it: zero is a value there, not a missing cell)")
        return getattr(lib(), fn), fn, (ctypes.byref(v), n_feat, n_samp), n_feat, n_samp, flags, (a, v)

    def scatter_csc_dev(self, d_values: int, d_indices: int, d_indptr: int, dtype: int, index_type: int, fill,
                        n_feat: int, n_samp: int, d_dst: int, dst_ld: int):
        """icikt_scatter_csc_dev: DEVICE arrays of a CSC matrix (DTYPE_* values, INDEX_* indices and column offsets) ->
        the column-major float64 device matrix prepare_dev takes, cells without an entry = fill.  Returns after the
        context's stream has been synchronised; malformed input raises."""
        self._chk(lib().icikt_scatter_csc_dev(self._h, ctypes.c_void_p(d_values or 0), ctypes.c_void_p(d_indices or 0),
                                              ctypes.c_void_p(d_indptr or 0), dtype, index_type, ctypes.c_double(fill),
                                              n_feat, n_samp, ctypes.c_void_p(d_dst or 0), dst_ld),
                  "icikt_scatter_csc_dev")

    def convert_dev(self, d_src: int, dtype: int, order: int, n_feat: int, n_samp: int, ld: int, d_dst: int,
                    dst_ld: int):
        """icikt_convert_dev: a device block of DTYPE_* cells in ORDER_* layout -> the column-major float64 device matrix
        prepare_dev takes (asynchronous on the context's stream)."""
        self._chk(lib().icikt_convert_dev(self._h, ctypes.c_void_p(d_src or 0), dtype, order, n_feat, n_samp, ld,
                                          ctypes.c_void_p(d_dst or 0), dst_ld), "icikt_convert_dev")

    def pairs(self, X, pi=None, pj=None, perspective="global", alternative="two.sided", continuity=False,
              flags: int = 0, want_counts: bool = True):
        """ici_split() over a host matrix (n_feat x n_samp, NaN = missing); pairs 0-based or None = all."""
        fn, fname, xargs, n_feat, n_samp, flags, _keep = self._entry("pairs", X, flags)
        if pi is None:
            P = n_samp * (n_samp - 1) // 2
            pi_a = pj_a = None
        else:
            pi_a = np.ascontiguousarray(pi, dtype=np.int32)
            pj_a = np.ascontiguousarray(pj, dtype=np.int32)
            P = pi_a.shape[0]
        alloc = pinned_empty if (flags & FLAG_HOST_PINNED) else np.empty   # (X is the caller's: pinned by the caller)
        out = alloc((P, 4), dtype=np.float64)
        cnt = alloc((P, len(CNT_FIELDS)), dtype=np.int64) if want_counts else None
        rsn = alloc(P, dtype=np.int32)
        if cnt is not None:
            cnt[...] = 0
        rsn[...] = 0
        alt = ALTERNATIVE.get(alternative, ALT_OTHER)
        self._chk(fn(self._h, *xargs, _ptr(pi_a), _ptr(pj_a), P, PERSPECTIVE[perspective], alt, int(bool(continuity)),
                     flags, _ptr(out), _ptr(cnt), _ptr(rsn)), fname)
        return out, cnt, rsn

    def matrix(self, X, global_na=None, pi=None, pj=None, perspective="global", alternative="two.sided",
               continuity=False, flags: int = 0, scale_max=True, diag_good=True, want_keep=True):
        """ici_kendalltau() below its argument checks in ONE call (icikt_matrix_f64): the exclusion rule, the pair
        kernels and scale_and_reshape all run on the device.  X: raw data (features x samples, F-ordered float64 is
        taken as is); global_na: the values setup_missing_matrix excludes (NaN = NA, Inf, finite values)."""
        fn = lib().icikt_matrix_f64 if self.f64_entries else \
            (lib().icikt_matrix_csc if is_sparse(X) else lib().icikt_matrix_in)
        return _matrix_call(fn, self._h, self._chk, X, global_na, pi, pj, perspective, alternative,
                            continuity, flags, scale_max, diag_good, want_keep, view=not self.f64_entries)

    def topk(self, X, k, global_na=None, perspective="global", alternative="two.sided", continuity=False,
             flags: int = 0, scale_max=True):
        """Every sample's k partners with the largest ICI-Kendall-tau, selected on the device (icikt_topk_f64): nothing
        of size S x S exists on either side.  X and global_na as matrix() takes them.  Returns (idx [S, k] int32, -1
        padded; vals5 [5, S, k]: cor, raw, pvalue, taumax, completeness, NA_real_ padded; n_valid [S]; max_taumax;
        reason_counts [5]).  A column's partners are ordered by raw descending (by the doubles' bits: -0.0 below +0.0),
        ties by the smaller index.  The argument checks are the library's: a bad k or perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("topk", X, flags))
        k = int(k)
        idx = sel.alloc((sel.n_samp, max(k, 0)), dtype=np.int32)
        vals = sel.alloc((5, sel.n_samp, max(k, 0)), dtype=np.float64)
        n_valid = np.zeros(sel.n_samp, dtype=np.int32)
        return idx, vals, n_valid, *sel(global_na, perspective, alternative, continuity, scale_max, (k,),
                                        (_ptr(idx), _ptr(vals), _ptr(n_valid)))

    def cross(self, query, reference, k=None, want_matrix=True, global_na=None, perspective="global",
              alternative="two.sided", continuity=False, flags: int = 0, scale_max=True):
        """Every column of `query` (n_feat x Sq) with every column of `reference` (n_feat x Sr) and nothing else
        (icikt_cross_in): the two matrices are read where they lie (input_view; they may differ in dtype and order; a
        sparse matrix is densified), global_na as matrix() takes it, applied to both.  want_matrix: the five Sq x Sr
        matrices; k: every query's k reference columns with the largest raw, in topk()'s order (raw descending by the
        doubles' bits, ties by the smaller reference index, an NA pair is no partner).  Returns (out5 [5, Sq, Sr]: cor,
        raw, pvalue, taumax, completeness, or None; idx [Sq, k] int32 reference column indices, -1 padded, or None;
        vals5 [5, Sq, k], NA_real_ padded, or None; n_valid [Sq] or None; max_taumax: the largest taumax of the
        rectangle, cor's denominator; reason_counts [5] over the rectangle).  A column that occurs in both matrices is a
        partner like any other.  The argument checks are the library's: a bad k, more than 65 535 columns in all or
        no output at all raises IciktError."""
        def dense(X):
            return csc_view(X).toarray() if is_sparse(X) else X
        if self.f64_entries:
            query, reference = (np.asfortranarray(dense(X), dtype=np.float64) for X in (query, reference))
        qa, qv, n_feat, Sq, flags = _view_arg(dense(query), flags)
        ra, rv, n_feat_r, Sr, flags = _view_arg(dense(reference), flags)
        if n_feat != n_feat_r:
            raise ValueError(f"`query` has {n_feat} rows and `reference` {n_feat_r}: the two must share their features")
        if self.f64_entries:
            fn, fname, xargs = lib().icikt_cross_f64, "icikt_cross_f64", (_ptr(qa), qv.ld, _ptr(ra), rv.ld)
        else:
            fn, fname, xargs = lib().icikt_cross_in, "icikt_cross_in", (ctypes.byref(qv), ctypes.byref(rv))
        sel = _SelectCall(self, (fn, fname, (*xargs, n_feat, Sq, Sr), n_feat, Sq, flags, (qa, qv, ra, rv)))
        total = Sq + (Sq & 1) + Sr
        fits = total <= TOPK_MAX_SAMPLES      # (the library refuses the others before it writes)
        out5 = sel.alloc((5, Sq, Sr) if fits else (5, 0, 0), dtype=np.float64) if want_matrix else None
        idx = vals = n_valid = None
        kk = 0
        if k is not None:
            kk = int(k)
            room = kk if 0 <= kk <= TOPK_MAX else 0
            idx = sel.alloc((Sq, room), dtype=np.int32)
            vals = sel.alloc((5, Sq, room), dtype=np.float64)
            n_valid = np.zeros(Sq, dtype=np.int32)
        return out5, idx, vals, n_valid, *sel(global_na, perspective, alternative, continuity, scale_max, (kk,),
                                              (_ptr(out5), _ptr(idx), _ptr(vals), _ptr(n_valid)))

    def _cross_view(self, X, flags):
        """(array, view, n_feat, n_samp, flags) of one matrix of cross / prepare_reference / cross_prepared: read where
        it lies, a sparse matrix densified; with f64_entries an F-ordered float64 copy."""
        if is_sparse(X):
            X = csc_view(X).toarray()
        if self.f64_entries:
            X = np.asfortranarray(X, dtype=np.float64)
        return _view_arg(X, flags)

    def prepare_reference(self, reference, query_capacity, global_na=None, flags: int = 0):
        """Upload and pre-pass `reference` (n_feat x Sr) once and keep it on this context (icikt_ref_prepare_in), with
        room for batches of up to `query_capacity` query columns: cross_prepared() then brings a batch alone.  global_na
        as matrix() takes it; it is recorded and applies to every batch.  Any other call on this context that computes
        pairs drops the reference (cross_prepared raises afterwards): give a reference that is to stay a context of its
        own.  The argument checks are the library's: a capacity below 1, or more than 65 535 columns in all, raises
        IciktError."""
        ra, rv, n_feat, Sr, flags = self._cross_view(reference, flags)
        gna = np.ascontiguousarray([] if global_na is None else np.atleast_1d(global_na), dtype=np.float64)
        tail = (n_feat, Sr, int(query_capacity), _ptr(gna) if gna.size else None, int(gna.size), flags)
        if self.f64_entries:
            self._chk(lib().icikt_ref_prepare_f64(self._h, _ptr(ra), rv.ld, *tail), "icikt_ref_prepare_f64")
        else:
            self._chk(lib().icikt_ref_prepare_in(self._h, ctypes.byref(rv), *tail), "icikt_ref_prepare_in")

    def reference_info(self):
        """(n_feat, n_reference, query_capacity) of the prepared reference; raises IciktError when there is none."""
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._chk(lib().icikt_ref_info(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "icikt_ref_info")
        return a.value, b.value, c.value

    def cross_prepared(self, query, k=None, want_matrix=True, ref_cls=None, n_class=0, perspective="global",
                       alternative="two.sided", continuity=False, flags: int = 0, scale_max=True):
        """cross() of `query` (n_feat x Sq) against the reference prepare_reference() left on this context
        (icikt_ref_cross_in): only the batch is uploaded and pre-passed, under the recorded global_na.  k and
        want_matrix as cross() takes them.  ref_cls: a class index in 0 .. n_class - 1 per reference column; with it
        the call also reduces every query's median to every class on the device.  Returns cross()'s six items and then
        (med2 [2, Sq, n_class]: cor, raw -- NA_real_ for a cell without a valid partner -- or None; n_valid [Sq,
        n_class] or None), views of the library's layout with the query index fastest.  The argument checks are the
        library's: no prepared reference, other rows than the reference's, a batch wider than the capacity, a class
        index out of range raise IciktError, and a refused call leaves the reference as it was."""
        qa, qv, n_feat, Sq, flags = self._cross_view(query, flags)
        _, Sr, _cap = self.reference_info()
        if self.f64_entries:
            fn, fname, xargs = lib().icikt_ref_cross_f64, "icikt_ref_cross_f64", (_ptr(qa), qv.ld)
        else:
            fn, fname, xargs = lib().icikt_ref_cross_in, "icikt_ref_cross_in", (ctypes.byref(qv),)
        alloc = pinned_empty if (flags & FLAG_HOST_PINNED) else np.empty
        out5 = alloc((5, Sq, Sr), dtype=np.float64) if want_matrix else None
        idx = vals = n_valid = cls_a = med2 = cls_n_valid = None
        kk = 0
        if k is not None:
            kk = int(k)
            room = kk if 0 <= kk <= TOPK_MAX else 0    # (the library refuses the others before it writes)
            idx = alloc((Sq, room), dtype=np.int32)
            vals = alloc((5, Sq, room), dtype=np.float64)
            n_valid = np.zeros(Sq, dtype=np.int32)
        n_class = int(n_class)
        if ref_cls is not None:
            cls_a = np.ascontiguousarray(ref_cls, dtype=np.int32)
            if cls_a.shape != (Sr,):
                raise ValueError("ref_cls must give one class per reference column")
            room = n_class if 1 <= n_class <= 65535 else 1
            med2 = np.empty((2, room, Sq), dtype=np.float64)
            cls_n_valid = np.zeros((room, Sq), dtype=np.int32)
        persp = PERSPECTIVE.get(perspective, perspective if isinstance(perspective, int) else -1)
        mx, rc5 = np.full(1, -np.inf), np.zeros(5, dtype=np.int64)
        self._chk(fn(self._h, *xargs, n_feat, Sq, kk, _ptr(cls_a), n_class, persp, ALTERNATIVE.get(alternative, ALT_OTHER),
                     int(bool(continuity)), flags, int(bool(scale_max)), _ptr(out5), _ptr(idx), _ptr(vals), _ptr(n_valid),
                     _ptr(med2), _ptr(cls_n_valid), _ptr(mx), _ptr(rc5)), fname)
        return (out5, idx, vals, n_valid, float(mx[0]), rc5,
                None if med2 is None else med2.transpose(0, 2, 1), None if cls_n_valid is None else cls_n_valid.T)

    def class_medians(self, X, cls=None, n_class=1, global_na=None, perspective="global", alternative="two.sided",
                      continuity=False, flags: int = 0, scale_max=True):
        """Every sample's median ICI-Kendall-tau over the other samples of its class, reduced on the device
        (icikt_class_medians_f64): only the within-class pairs are computed, and nothing of size S x S exists on either
        side.  cls: a class index in 0 .. n_class - 1 per column (None: one class); X and global_na as matrix() takes
        them.  Returns (med2 [2, S]: cor, raw -- NA_real_ for a sample without a valid partner; n_valid [S];
        max_taumax: the largest taumax of the COMPUTED pairs, cor's denominator; reason_counts [5] over those pairs).
        The argument checks are the library's: a class index out of range or a bad perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("class_medians", X, flags))
        cls_a = _class_arg(cls, sel.n_samp)
        med2 = np.empty((2, sel.n_samp), dtype=np.float64)
        n_valid = np.zeros(sel.n_samp, dtype=np.int32)
        return med2, n_valid, *sel(global_na, perspective, alternative, continuity, scale_max,
                                   (_ptr(cls_a), int(n_class)), (_ptr(med2), _ptr(n_valid)))

    def class_matrix(self, X, cls=None, n_class=1, global_na=None, perspective="global", alternative="two.sided",
                     continuity=False, flags: int = 0, scale_max=True):
        """Every sample's median ICI-Kendall-tau to every class, reduced on the device (icikt_class_matrix_f64): all
        pairs are computed, and nothing of size S x S exists on the host or as five planes on the device.  cls: a class
        index in 0 .. n_class - 1 per column (None: one class, a table of one column); X and global_na as matrix()
        takes them.  Returns (med2 [2, S, n_class]: cor, raw -- NA_real_ for a cell without a valid partner; n_valid
        [S, n_class]; max_taumax: the largest taumax of ALL pairs, cor's denominator; reason_counts [5] over all
        pairs).  The arrays are views of the library's layout, the sample index fastest.  The argument checks are the
        library's: a class index out of range, more than 65 535 classes or a bad perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("class_matrix", X, flags))
        cls_a = _class_arg(cls, sel.n_samp)
        if cls_a is None:
            n_class = 1
        n_class = int(n_class)
        room = n_class if 1 <= n_class <= 65535 else 1    # (the library refuses the others before it writes)
        med2 = np.empty((2, room, sel.n_samp), dtype=np.float64)
        n_valid = np.zeros((room, sel.n_samp), dtype=np.int32)
        return med2.transpose(0, 2, 1), n_valid.T, *sel(global_na, perspective, alternative, continuity, scale_max,
                                                        (_ptr(cls_a), n_class), (_ptr(med2), _ptr(n_valid)))

    def quantiles(self, X, probs=(), breaks=None, cls=None, n_class=1, global_na=None, perspective="global",
                  alternative="two.sided", continuity=False, flags: int = 0, scale_max=True):
        """Exact quantiles (R's type 7) and a histogram of raw over ALL pairs, reduced on the device
        (icikt_quantiles_f64): nothing of size S x S exists on the host or as five planes on the device.  probs: up to
        32 values in [0, 1]; breaks: strictly increasing bin edges (numpy.histogram's bins), None for no histogram;
        cls: a class index in 0 .. n_class - 1 per column, which splits the result into the groups all / within-class
        / between-class pairs (None: the one group of all pairs).  Returns (q2 [2, n_group, n_probs]: cor, raw --
        NA_real_ for a group without a valid pair; order2 [n_group, n_probs, 2]: the two order statistics each
        quantile interpolates; n_valid, n_na [n_group] int64; hist [n_group, n_bins] int64; outside [n_group, 2]:
        values below the first and above the last break; max_taumax; reason_counts [5]).  The argument checks are the
        library's: a bad prob, break, class index or perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("quantiles", X, flags))
        cls_a = _class_arg(cls, sel.n_samp)
        probs_a = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)).ravel())
        breaks_a = np.empty(0) if breaks is None else np.ascontiguousarray(np.atleast_1d(breaks), dtype=np.float64).ravel()
        n_probs, n_breaks = int(probs_a.size), int(breaks_a.size)
        n_group = 1 if cls_a is None else 3
        q2 = np.empty((2, n_group, n_probs), dtype=np.float64)
        order2 = np.empty((n_group, n_probs, 2), dtype=np.float64)
        n_valid = np.zeros(n_group, dtype=np.int64)
        n_na = np.zeros(n_group, dtype=np.int64)
        hist = np.zeros((n_group, max(n_breaks - 1, 0)), dtype=np.int64)
        outside = np.zeros((n_group, 2), dtype=np.int64)
        return q2, order2, n_valid, n_na, hist, outside, *sel(
            global_na, perspective, alternative, continuity, scale_max, (_ptr(cls_a), int(n_class)),
            (_ptr(probs_a) if n_probs else None, n_probs, _ptr(breaks_a) if n_breaks else None, n_breaks,
             _ptr(q2) if n_probs else None, _ptr(order2) if n_probs else None, _ptr(n_valid), _ptr(n_na),
             _ptr(hist) if n_breaks > 1 else None, _ptr(outside)))

    def padjust(self, X, method, alpha, max_table=0, global_na=None, perspective="global", alternative="two.sided",
                continuity=False, flags: int = 0):
        """R's p.adjust over the p-values of ALL pairs, sorted, scanned and cut on the device (icikt_padjust_f64):
        nothing of size S x S exists on the host or as five planes on the device.  method: "bonferroni", "holm",
        "hochberg" or "BH" (or the ICIKT_ADJUST_* code); alpha: up to 16 levels in [0, 1]; X and global_na as matrix()
        takes them.  The tests are the pairs with reason code 0 and a p-value that is not NaN.  Returns (n_tests [2]
        int64: tests, other pairs; n_rejected [n_alpha] int64: tests whose adjusted p is <= alpha; p_cutoff [n_alpha]:
        the largest rejected raw p -- edges(max_pvalue=p_cutoff) selects exactly the rejected pairs --, NA_real_ when
        none; table [2, t]: the distinct p-values among the rejected tests of the largest alpha, ascending, and their
        adjusted values, t = min(n_table, max_table); n_table: ALL distinct values, so n_table > max_table says the
        table is truncated (call again with room); max_taumax; reason_counts [5]).  The argument checks are the
        library's: a bad method, alpha or perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("padjust", X, flags))
        code = ADJUST.get(method, method if isinstance(method, (int, np.integer)) else -1)
        alpha_a = np.ascontiguousarray(np.atleast_1d(np.asarray(alpha, dtype=np.float64)).ravel())
        n_alpha = int(alpha_a.size)
        max_table = int(max_table)
        room = max(0, min(max_table, sel.n_samp * (sel.n_samp - 1) // 2))   # (no more distinct p-values than pairs)
        n_tests = np.zeros(2, dtype=np.int64)
        n_rej = np.zeros(max(n_alpha, 1), dtype=np.int64)
        cutoff = np.empty(max(n_alpha, 1), dtype=np.float64)
        table = np.empty((2, room), dtype=np.float64) if room else None
        n_table = np.zeros(1, dtype=np.int64)
        tail = sel(global_na, perspective, alternative, continuity, None, (),
                   (int(code), _ptr(alpha_a) if n_alpha else None, n_alpha, room if max_table >= 0 else max_table,
                    _ptr(n_tests), _ptr(n_rej), _ptr(cutoff), _ptr(table), _ptr(n_table)))
        t = min(int(n_table[0]), room)
        table = table[:, :t] if room else np.empty((2, 0), dtype=np.float64)
        return n_tests, n_rej[:n_alpha], cutoff[:n_alpha], table, int(n_table[0]), *tail

    def mst(self, X, min_raw=None, global_na=None, perspective="global", alternative="two.sided", continuity=False,
            flags: int = 0, scale_max=True):
        """The maximum spanning forest of the samples under raw -- their single-linkage clustering -- found on the
        device (icikt_mst_f64): all pairs are computed, and nothing of size S x S exists on the host or as five planes
        on the device.  A pair is a candidate edge iff its raw is not NA and, with min_raw, raw >= min_raw; the strict
        edge order is the larger raw first (-0 equal to +0), equal raw by the smaller combn index, so the forest is
        unique.  X and global_na as matrix() takes them.  Returns (ti, tj [n_tree] int32: the edges i < j in the strict
        order, which is the single-linkage merge order; vals5 [5, n_tree]: cor, raw, pvalue, taumax, completeness;
        component [S] int32: the components of the candidate graph, numbered in order of their smallest sample;
        n_components; n_rounds: the Boruvka rounds run; max_taumax; reason_counts [5]) with n_tree + n_components == S.
        The argument checks are the library's: a bad perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("mst", X, flags))
        n_samp, room = sel.n_samp, sel.tree_room()
        ti = np.empty(max(room, 1), dtype=np.int32)
        tj = np.empty(max(room, 1), dtype=np.int32)
        vals = np.empty((5, max(room, 1)), dtype=np.float64)
        component = np.zeros(max(n_samp, 1), dtype=np.int32)
        n_tree = np.zeros(1, dtype=np.int64)
        n_comp = np.zeros(1, dtype=np.int64)
        n_rounds = np.zeros(1, dtype=np.int32)
        tail = sel(global_na, perspective, alternative, continuity, scale_max, (),
                   (float("nan") if min_raw is None else float(min_raw), _ptr(ti), _ptr(tj), _ptr(vals), _ptr(n_tree),
                    _ptr(component), _ptr(n_comp), _ptr(n_rounds)))
        m = int(n_tree[0])
        # (the library's planes are room apart: one row of vals each when room >= 1)
        return ti[:m], tj[:m], vals[:, :m], component[:n_samp], int(n_comp[0]), int(n_rounds[0]), *tail

    def hclust(self, X, method="complete", min_raw=None, global_na=None, perspective="global", alternative="two.sided",
               continuity=False, flags: int = 0, scale_max=True):
        """Agglomerative clustering of the samples under raw with "complete", "average" or "single" linkage, run on the
        device (icikt_hclust_f64): all pairs are computed, and nothing of size S x S exists on the host or as five
        planes on the device.  A cluster lives in the slot of its smallest sample; each step merges the best live pair
        of clusters a < b into a, in the strict order larger similarity first (-0 equal to +0), then smaller a, then
        smaller b; the merged cluster's similarity to another is NA if either old one is, else the smaller (complete),
        the larger (single) or the size-weighted mean (average: two products, two sums, one division, each rounded
        once) of the two.  Merging ends at the first step whose best similarity is NA or below min_raw.  method may
        also be the library's code; X and global_na as matrix() takes them.  Returns (ma, mb, msize [n_merges] int32:
        the slots a < b and the new cluster's samples, in merge order; mraw, mcor [n_merges]; component [S] int32: the
        clusters that are left, numbered in order of their smallest sample; n_components; max_taumax; reason_counts
        [5]) with n_merges + n_components == S.  The argument checks are the library's: an unknown method or a bad
        perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("hclust", X, flags))
        code = HCLUST.get(method, -1) if isinstance(method, str) else int(method)
        n_samp, room = sel.n_samp, sel.tree_room()
        ma =np.empty(max(room, 1), dtype=np.int32)
        mb = np.empty(max(room, 1), dtype=np.int32)
        msize = np.empty(max(room, 1), dtype=np.int32)
        mraw = np.empty(max(room, 1), dtype=np.float64)
        mcor = np.empty(max(room, 1), dtype=np.float64)
        component = np.zeros(max(n_samp, 1), dtype=np.int32)
        n_merges = np.zeros(1, dtype=np.int64)
        n_comp = np.zeros(1, dtype=np.int64)
        tail = sel(global_na, perspective, alternative, continuity, scale_max, (),
                   (code, float("nan") if min_raw is None else float(min_raw), _ptr(ma), _ptr(mb), _ptr(msize), _ptr(mraw),
                    _ptr(mcor), _ptr(n_merges), _ptr(component), _ptr(n_comp)))
        m = int(n_merges[0])
        return ma[:m], mb[:m], msize[:m], mraw[:m], mcor[:m], component[:n_samp], int(n_comp[0]), *tail

    def anosim(self, X, cls=None, n_class=1, perm_cls=None, global_na=None, perspective="global",
               alternative="two.sided", continuity=False, flags: int = 0):
        """ANOSIM of the classes under the dissimilarity 1 - raw with its permutation sums, on the device
        (icikt_anosim_f64): all pairs are computed, ranked and summed there, and nothing of size S x S exists on the
        host or as five planes on the device.  cls: a class index in 0 .. n_class - 1 per column (None: one class);
        perm_cls: [n_perm, S] class indices, the labellings to compare with (None: none); X and global_na as matrix()
        takes them.  Returns (n_pairs [2] int64: values M, NA pairs; w2, nw [1 + n_perm] int64: the doubled rank sum and
        the count of the within-class values, index 0 the observed labelling; n_ge: the permutations whose R is defined
        and >= the observed R, compared exactly; n_undefined: the permutations without an R; class_w2, class_nw
        [n_class] int64: the observed sums per class; max_taumax; reason_counts [5]).  api.anosim_statistic turns a
        (M, w2, nw) into the statistic.  The argument checks are the library's: a label out of range, more than 65 535 classes or a
        bad perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("anosim", X, flags))
        cls_a, n_class, perm_a, n_perm, room, n_lab = _labellings_arg(cls, n_class, perm_cls, sel.n_samp)
        n_pairs = np.zeros(2, dtype=np.int64)
        w2 = np.zeros(n_lab, dtype=np.int64)
        nw = np.zeros(n_lab, dtype=np.int64)
        n_ge = np.zeros(1, dtype=np.int64)
        n_undef = np.zeros(1, dtype=np.int64)
        class_w2 = np.zeros(room, dtype=np.int64)
        class_nw = np.zeros(room, dtype=np.int64)
        tail = sel(global_na, perspective, alternative, continuity, None, (),
                   (_ptr(cls_a), n_class, _ptr(perm_a) if n_perm else None, n_perm, _ptr(n_pairs), _ptr(w2), _ptr(nw),
                    _ptr(n_ge), _ptr(n_undef), _ptr(class_w2), _ptr(class_nw)))
        return n_pairs, w2, nw, int(n_ge[0]), int(n_undef[0]), class_w2, class_nw, *tail

    def permanova(self, X, cls=None, n_class=1, perm_cls=None, global_na=None, perspective="global",
                  alternative="two.sided", continuity=False, flags: int = 0):
        """PERMANOVA's integer sums of the classes under the dissimilarity 1 - raw, on the device
        (icikt_permanova_f64): all pairs are computed, their (1 - raw)^2 turned into the fixed-point integers q
        (csrc/icikt_fixed.h) and summed there per class and labelling.  cls, n_class, perm_cls, X and global_na as
        anosim() takes them.  Returns (n_pairs [2] int64: values, NA pairs; Q: the sum of q over all values, a Python
        int; class_q [1 + n_perm, n_class] of Python ints (dtype object): A_c of every labelling, row 0 the observed
        one, all 0 when there is an NA pair; max_taumax; reason_counts [5]).  The limbs of the C ABI are combined here:
        A = hi 2^32 + lo.  api.permanova_statistic turns (S, Q, a row of class_q, the row's class sizes) into the
        statistic.  The argument checks are the library's: a label out of range, more than 65 535 classes, more than
        PERMANOVA_MAX_CELLS cells or a bad perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("permanova", X, flags))
        cls_a, n_class, perm_a, n_perm, room, n_lab = _labellings_arg(cls, n_class, perm_cls, sel.n_samp)
        if n_lab * room > PERMANOVA_MAX_CELLS:
            n_lab = 1
        n_pairs = np.zeros(2, dtype=np.int64)
        q_total = np.zeros(2, dtype=np.int64)
        bins_lo = np.zeros((n_lab, room), dtype=np.int64)
        bins_hi = np.zeros((n_lab, room), dtype=np.int64)
        tail = sel(global_na, perspective, alternative, continuity, None, (),
                   (_ptr(cls_a), n_class, _ptr(perm_a) if n_perm else None, n_perm, _ptr(n_pairs), _ptr(q_total),
                    _ptr(bins_lo), _ptr(bins_hi)))
        class_q = bins_hi.astype(object) * (1 << 32) + bins_lo.astype(object)
        return n_pairs, (int(q_total[1]) << 32) + int(q_total[0]), class_q, *tail

    def permdisp(self, X, cls=None, n_class=1, global_na=None, perspective="global", alternative="two.sided",
                 continuity=False, flags: int = 0):
        """PERMDISP's integer table of the classes under the dissimilarity 1 - raw, on the device (icikt_permdisp_f64):
        all pairs are computed, their (1 - raw)^2 turned into PERMANOVA's fixed-point integers q (csrc/icikt_fixed.h)
        and summed there per sample and class.  cls, n_class, X and global_na as class_matrix() takes them.  Returns
        (n_pairs [2] int64: values, NA pairs; Q: the sum of q over all values, a Python int; T [S, n_class] of Python
        ints (dtype object): T[i][c] the sum of q_ij over the samples j != i of class c, as summed also when a pair is
        NA (it adds 0); max_taumax; reason_counts [5]).  The limbs of the C ABI are combined here: T = hi 2^32 + lo.
        api.permdisp_distance and api.permdisp_statistic turn the table into the distances to the class centroids and
        their ANOVA F.  The argument checks are the library's: a label out of range, more than 65 535 classes, more
        than PERMDISP_MAX_CELLS cells or a bad perspective raises IciktError."""
        sel = _SelectCall(self, self._entry("permdisp", X, flags))
        cls_a = _class_arg(cls, sel.n_samp)
        n_class = int(n_class) if cls_a is not None else 1
        room = n_class if 1 <= n_class <= 65535 and sel.n_samp * n_class <= PERMDISP_MAX_CELLS else 1
        n_pairs = np.zeros(2, dtype=np.int64)
        q_total = np.zeros(2, dtype=np.int64)
        t_lo = np.zeros((sel.n_samp, room), dtype=np.int64)
        t_hi = np.zeros((sel.n_samp, room), dtype=np.int64)
        tail = sel(global_na, perspective, alternative, continuity, None, (),
                   (_ptr(cls_a), n_class, _ptr(n_pairs), _ptr(q_total), _ptr(t_lo), _ptr(t_hi)))
        return n_pairs, (int(q_total[1]) << 32) + int(q_total[0]), _limbs_to_ints(t_lo, t_hi), *tail

    def mantel(self, X, other, method="pearson", perms=None, global_na=None, perspective="global",
               alternative="two.sided", continuity=False, flags: int = 0):
        """The Mantel test's integer sums of the dissimilarity 1 - raw against another matrix of the same samples, on
        the device (icikt_mantel_f64): all pairs are computed and turned into integers below 2^32 -- their doubled ranks
        (method "spearman") or fixed-point values (method "pearson", csrc/icikt_mantel.h) -- as `other` is, and
        T = sum x_ij y_pi(i)pi(j) is summed there for the identity and every permutation.  other: [P] finite doubles,
        one per pair i < j in combn order (scipy's squareform order); perms: [n_perm, S] sample indices, every row a
        permutation of 0 .. S - 1 (None: none); X and global_na as matrix() takes them.  Returns (n_pairs [2] int64:
        values, NA pairs; T [1 + n_perm] of Python ints (dtype object), index 0 the identity; moments: (Sx, Sxx, Sy,
        Syy) as Python ints; n_ge, n_le: the permutations with T >= / <= T[0], compared exactly; max_taumax;
        reason_counts [5]).  With an NA pair every T and moment is 0.  The limbs of the C ABI are combined here.
        api.mantel_statistic turns (P, T, Sx, Sxx, Sy, Syy) into r.  The argument checks are the library's: a value of
        other that is not finite, a row of perms that is no permutation or a bad method raises IciktError."""
        sel = _SelectCall(self, self._entry("mantel", X, flags))
        S = sel.n_samp
        other_a = np.ascontiguousarray(other, dtype=np.float64)
        if other_a.shape != (S * (S - 1) // 2 if S > 1 else 0,):
            raise ValueError("other must be [S (S - 1) / 2]: one value per pair in combn order")
        if perms is None:
            perm_a, n_perm = None, 0
        else:
            perm_a = np.ascontiguousarray(perms, dtype=np.int32)
            if perm_a.ndim != 2 or perm_a.shape[1] != S:
                raise ValueError("perms must be [n_perm, S]: one sample index per column in every row")
            n_perm = int(perm_a.shape[0])
        n_lab = 1 + (n_perm if n_perm <= MANTEL_MAX_PERM else 0)
        n_pairs = np.zeros(2, dtype=np.int64)
        t_lo = np.zeros(n_lab, dtype=np.int64)
        t_hi = np.zeros(n_lab, dtype=np.int64)
        moments = np.zeros(8, dtype=np.int64)
        n_ge = np.zeros(1, dtype=np.int64)
        n_le = np.zeros(1, dtype=np.int64)
        code = MANTEL.get(method, method if isinstance(method, int) else -1)
        tail = sel(global_na, perspective, alternative, continuity, None, (),
                   (_ptr(other_a) if other_a.size else None, code, _ptr(perm_a) if n_perm else None, n_perm, _ptr(n_pairs),
                    _ptr(t_lo), _ptr(t_hi), _ptr(moments), _ptr(n_ge), _ptr(n_le)))
        T = t_hi.astype(object) * (1 << 32) + t_lo.astype(object)
        mom = tuple((int(moments[2 * k + 1]) << 32) + int(moments[2 * k]) for k in range(4))
        return n_pairs, T, mom, int(n_ge[0]), int(n_le[0]), *tail

    def pcoa_apply_dev(self, d_G: int, d_V: int, n_samp: int, b: int, d_W: int):
        """icikt_pcoa_apply_dev: W = G V on DEVICE arrays (G row-major [S, S]; V and W [b, S], a block's column c in row
        c), asynchronous on the context's stream."""
        self._chk(lib().icikt_pcoa_apply_dev(self._h, ctypes.c_void_p(d_G or 0), ctypes.c_void_p(d_V or 0), n_samp, b,
                                             ctypes.c_void_p(d_W or 0)), "icikt_pcoa_apply_dev")

    def pcoa(self, X, k=10, tol=1e-8, max_basis=None, seed=0, return_gower=False, global_na=None, perspective="global",
             alternative="two.sided", continuity=False, flags: int = 0, start=None):
        """The principal coordinates of the samples under the dissimilarity 1 - raw, on the device (icikt_pcoa_f64): all
        pairs are computed, their (1 - raw)^2 turned into PERMANOVA's fixed-point integers q (csrc/icikt_fixed.h), the
        Gower-centred S x S table G built from them and its k algebraically largest eigenpairs found there by a block
        Krylov iteration -- no S x S matrix reaches the host unless return_gower asks for G.  tol: the iteration stops
        when every residual |G y - theta y| is within tol |G|_F; max_basis: the most basis columns (None: min(S, max(8 k,
        128)); at most PCOA_MAX_BASIS); the start block [k, S] is `start`, or standard normals of
        numpy.random.default_rng(seed).  X and global_na as matrix() takes them.  Returns (n_pairs [2] int64: values, NA
        pairs; Q: the sum of q over all values, a Python int; R [S] of Python ints (dtype object): the row sums of q;
        eigenvalues [k], descending; vectors [S, k], orthonormal columns, each with its component of largest magnitude
        positive; residuals [k]; frobenius: |G|_F; min_ritz: the smallest Ritz value of the last projected problem;
        n_basis; n_apply; converged; G [S, S] or None; max_taumax; reason_counts [5]).  With an NA pair every double is
        NA_real_ and the integers are as summed.  The argument checks are the library's: fewer than two samples, a k
        outside 1 .. min(S - 1, PCOA_MAX_K), a tol that is not positive or a max_basis below k raises IciktError."""
        sel = _SelectCall(self, self._entry("pcoa", X, flags))
        S, k = sel.n_samp, int(k)
        room = k if 1 <= k <= PCOA_MAX_K else 1
        if start is None:
            start = np.random.default_rng(seed).standard_normal((room, max(S, 1)))
        start = np.ascontiguousarray(start, dtype=np.float64)
        if start.shape != (room, max(S, 1)):
            raise ValueError("start must be [k, S]: one row per column of the start block")
        n_pairs = np.zeros(2, dtype=np.int64)
        q_total = np.zeros(2, dtype=np.int64)
        row_lo = np.zeros(max(S, 1), dtype=np.int64)
        row_hi = np.zeros(max(S, 1), dtype=np.int64)
        eigenvalues = np.zeros(room, dtype=np.float64)
        vectors = sel.alloc((room, max(S, 1)), dtype=np.float64)
        residuals = np.zeros(room, dtype=np.float64)
        frobenius, min_ritz = np.zeros(1, dtype=np.float64), np.zeros(1, dtype=np.float64)
        solver = np.zeros(3, dtype=np.int64)
        gower = sel.alloc((max(S, 1), max(S, 1)), dtype=np.float64) if return_gower else None
        tail = sel(global_na, perspective, alternative, continuity, None, (),
                   (k, float(tol), 0 if max_basis is None else (int(max_basis) if int(max_basis) > 0 else -1), _ptr(start), _ptr(n_pairs), _ptr(q_total),
                    _ptr(row_lo), _ptr(row_hi), _ptr(eigenvalues), _ptr(vectors), _ptr(residuals), _ptr(frobenius),
                    _ptr(min_ritz), _ptr(solver), _ptr(gower)))
        return (n_pairs, (int(q_total[1]) << 32) + int(q_total[0]), _limbs_to_ints(row_lo[:S], row_hi[:S]), eigenvalues,
                vectors[:, :S].T, residuals, float(frobenius[0]), float(min_ritz[0]), int(solver[0]), int(solver[1]),
                bool(solver[2]), gower, *tail)

    def edges(self, X, min_raw=None, max_pvalue=None, min_completeness=None, absolute=False, max_edges=0,
              global_na=None, perspective="global", alternative="two.sided", continuity=False, flags: int = 0,
              scale_max=True, want_degree=True):
        """Every pair i < j whose raw (fabs(raw) with absolute), p-value and completeness pass the bounds that are not
        None, in combn order, compacted on the device (icikt_edges_f64): nothing of size S x S exists on either side.
        The bounds apply to raw, not to cor.  X and global_na as matrix() takes them.  Returns (ei, ej [m] int32; vals5
        [5, m]: cor, raw, pvalue, taumax, completeness; n_edges: ALL matching pairs; degree [S] int64 or None;
        max_taumax; reason_counts [5]) with m = min(n_edges, max_edges): max_edges = 0 only counts, and n_edges >
        max_edges says the list is truncated (call again with room).  The argument checks are the library's."""
        sel = _SelectCall(self, self._entry("edges", X, flags))
        n_samp = sel.n_samp
        max_edges = int(max_edges)
        rule = edge_rule(min_raw, max_pvalue, min_completeness, absolute)
        room = max(0, min(max_edges, n_samp * (n_samp - 1) // 2))   # (the library writes no slot past the triangle)
        ei = sel.alloc(room, dtype=np.int32) if room else None
        ej = sel.alloc(room, dtype=np.int32) if room else None
        vals = sel.alloc((5, room), dtype=np.float64) if room else None
        n_edges = np.zeros(1, dtype=np.int64)
        degree = np.zeros(n_samp, dtype=np.int64) if want_degree else None
        tail = sel(global_na, perspective, alternative, continuity, scale_max, (ctypes.byref(rule),),
                   (room if max_edges >= 0 else max_edges, _ptr(ei), _ptr(ej), _ptr(vals), _ptr(n_edges), _ptr(degree)))
        m = min(int(n_edges[0]), room)
        if room:
            ei, ej, vals = ei[:m], ej[:m], vals[:, :m]
        else:
            ei, ej, vals = np.empty(0, np.int32), np.empty(0, np.int32), np.empty((5, 0), np.float64)
        return ei, ej, vals, int(n_edges[0]), degree, *tail

    def pairs_complete(self, X, pi, pj, alternative="two.sided", continuity=False, flags: int = 0,
                       want_counts: bool = False):
        """kt_fast(use = "pairwise.complete.obs"): per pair, rows with a missing value in either vector are dropped."""
        fn, fname, xargs, n_feat, n_samp, flags, _keep = self._entry("pairs_complete", X, flags)
        pi_a = np.ascontiguousarray(pi, dtype=np.int32)
        pj_a = np.ascontiguousarray(pj, dtype=np.int32)
        P = pi_a.shape[0]
        out = np.empty((P, 4), dtype=np.float64)
        cnt = np.zeros((P, len(CNT_FIELDS)), dtype=np.int64) if want_counts else None
        rsn = np.zeros(P, dtype=np.int32)
        alt = ALTERNATIVE.get(alternative, ALT_OTHER)
        self._chk(fn(self._h, *xargs, _ptr(pi_a), _ptr(pj_a), P, alt, int(bool(continuity)), flags, _ptr(out), _ptr(cnt),
                     _ptr(rsn)), fname)
        return out, cnt, rsn

    def cor_pairs(self, X, pi, pj, method="pearson", pairwise=False, alternative="two.sided", continuity=False,
                  flags: int = 0):
        """cor_fast's pairs (icikt_cor_pairs_f64): (out3 [P, 3]: rho, p-value, n_values; reasons [P], ICIKT_COR_*)."""
        fn, fname, xargs, n_feat, n_samp, flags, _keep = self._entry("cor_pairs", X, flags)
        pi_a = np.ascontiguousarray(pi, dtype=np.int32)
        pj_a = np.ascontiguousarray(pj, dtype=np.int32)
        P = pi_a.shape[0]
        out = np.empty((P, 3), dtype=np.float64)
        rsn = np.zeros(P, dtype=np.int32)
        self._chk(fn(self._h, *xargs, _ptr(pi_a), _ptr(pj_a), P, METHOD[method], int(bool(pairwise)),
                     ALTERNATIVE[alternative], int(bool(continuity)), flags, _ptr(out), _ptr(rsn)), fname)
        return out, rsn

    # -- missing-value diagnostics (icikt_col_medians_f64 / icikt_censor_counts_f64 / icikt_rank_order_f64) --------
    def _diag_input(self, name, X, global_na, flags):
        gna = np.ascontiguousarray([] if global_na is None else np.atleast_1d(global_na), dtype=np.float64)
        return self._entry(name, X, flags, ld_floor=1), gna

    def col_medians(self, X, na_rm=False, global_na=None, flags: int = 0):
        """stats::median of every column (NaN = NA; global_na: cells the rule excludes as well)."""
        (fn, fname, xargs, n_feat, n_samp, flags, _keep), gna = self._diag_input("col_medians", X, global_na, flags)
        out = np.empty(n_samp, dtype=np.float64)
        self._chk(fn(self._h, *xargs, _ptr(gna) if gna.size else None, int(gna.size), int(bool(na_rm)), flags, _ptr(out)),
                  fname)
        return out

    def censor_counts(self, X, global_na, cls, n_class: int, flags: int = 0, want_medians: bool = False):
        """test_left_censorship's per-class counts: (trials [n_class], success [n_class], n_excluded, medians)."""
        (fn, fname, xargs, n_feat, n_samp, flags, _keep), gna = self._diag_input("censor_counts", X, global_na, flags)
        cls_a = np.ascontiguousarray(cls, dtype=np.int32)
        if cls_a.shape != (n_samp,):
            raise ValueError("cls must give one class per column")
        trials = np.zeros(n_class, dtype=np.int64)
        success = np.zeros(n_class, dtype=np.int64)
        n_ex = np.zeros(1, dtype=np.int64)
        med = np.empty(n_samp, dtype=np.float64) if want_medians else None
        self._chk(fn(self._h, *xargs, _ptr(gna) if gna.size else None, int(gna.size), _ptr(cls_a), int(n_class), flags,
                     _ptr(trials), _ptr(success), _ptr(n_ex), _ptr(med)), fname)
        return trials, success, int(n_ex[0]), med

    def rank_order(self, X, global_na, cols, flags: int = 0, want_data: bool = True, n_feat: int | None = None):
        """rank_order_data for the columns `cols` of X: dict of n_kept, n_na, median_rank, row_order, col_order and
        (want_data) original / ordered (n_kept x len(cols)).  n_feat: only the first n_feat rows of X count (X then
        passes with its own row count as the leading dimension)."""
        (fn, fname, xargs, rows, n_samp, flags, _keep), gna = self._diag_input("rank_order", X, global_na, flags)
        n_feat = rows if n_feat is None else int(n_feat)
        xargs = (xargs[0], n_feat) + tuple(xargs[2:])   # (the view / ld keeps X's own row count as the leading dimension)
        cols_a = np.ascontiguousarray(cols, dtype=np.int32)
        n_cols = cols_a.shape[0]
        n_kept = np.zeros(1, dtype=np.int64)
        n_na = np.empty(max(n_feat, 1), dtype=np.int32)
        med = np.empty(max(n_feat, 1), dtype=np.float64)
        rord = np.empty(max(n_feat, 1), dtype=np.int32)
        cord = np.empty(max(n_cols, 1), dtype=np.int32)
        orig = np.empty(max(n_feat * n_cols, 1), dtype=np.float64) if want_data else None
        ordd = np.empty(max(n_feat * n_cols, 1), dtype=np.float64) if want_data else None
        self._chk(fn(self._h, *xargs, _ptr(gna) if gna.size else None, int(gna.size), _ptr(cols_a), n_cols, flags,
                     _ptr(n_kept), _ptr(n_na), _ptr(med), _ptr(rord), _ptr(cord), _ptr(orig), _ptr(ordd)), fname)
        k = int(n_kept[0])
        out = {"n_kept": k, "n_na": n_na[:n_feat], "median_rank": med[:n_feat], "row_order": rord[:k],
               "col_order": cord[:n_cols]}
        if want_data:
            out["original"] = orig[:k * n_cols].reshape((k, n_cols), order="F")
            out["ordered"] = ordd[:k * n_cols].reshape((k, n_cols), order="F")
        return out

    def pair(self, x, y, perspective="local", alternative="two.sided", continuity=False, flags: int = 0):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        out = np.empty(4, dtype=np.float64)
        cnt = np.zeros(len(CNT_FIELDS), dtype=np.int64)
        rsn = np.zeros(1, dtype=np.int32)
        alt = ALTERNATIVE.get(alternative, ALT_OTHER)
        self._chk(lib().icikt_pair_f64(self._h, _ptr(x), _ptr(y), x.shape[0], PERSPECTIVE[perspective], alt,
                                       int(bool(continuity)), flags, _ptr(out), _ptr(cnt), _ptr(rsn)),
                  "icikt_pair_f64")
        return out, dict(zip(CNT_FIELDS, cnt.tolist())), int(rsn[0])

    def missingness(self, X, pi, pj):
        fn, fname, xargs, n_feat, n_samp, _flags, _keep = self._entry("missingness", X)
        pi_a = np.ascontiguousarray(pi, dtype=np.int32)
        pj_a = np.ascontiguousarray(pj, dtype=np.int32)
        out = np.zeros(pi_a.shape[0], dtype=np.int64)
        self._chk(fn(self._h, *xargs, _ptr(pi_a), _ptr(pj_a), pi_a.shape[0], _ptr(out)), fname)
        return out


def cost_blocks(col_cost, n_blocks: int, pj=None, max_block: int = 0):
    """The cost-weighted cut of the pair list (icikt_cost_blocks; host arithmetic, no device): bounds[0 .. n_blocks]."""
    cost = np.ascontiguousarray(col_cost, dtype=np.uint32)
    pj_a = None if pj is None else np.ascontiguousarray(pj, dtype=np.int32)
    b = np.zeros(n_blocks + 1, dtype=np.int64)
    rc = lib().icikt_cost_blocks(_ptr(cost), cost.shape[0], _ptr(pj_a), -1 if pj_a is None else pj_a.shape[0], n_blocks,
                                 int(max_block), _ptr(b))
    if rc != SUCCESS:
        raise IciktError(f"icikt_cost_blocks failed (code {rc})")
    return b.tolist()


EXCHANGE = {"auto": 0, "rccl": 1, "copy": 2}
MULTI_PHASES = ("prepare", "exchange", "pairs", "gather")


class MultiContext:
    """Several MI355X behind one call (icikt_multi): one host thread per device inside the library, column-sharded
    pre-pass, RCCL all-gather / gather over xGMI."""

    def __init__(self, devices=None, n_gpu: int | None = None, exchange: str = "auto"):
        if devices is None:
            devices = list(range(int(n_gpu or 1)))
        self.devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        self._h = ctypes.c_void_p()
        rc = lib().icikt_multi_create(arr, len(self.devices), EXCHANGE[exchange], ctypes.byref(self._h))
        if rc == E_NO_DEVICE:
            raise IciktError("no usable HIP device: icikendalltau_amd computes on MI355X only (no CPU fallback)")
        if rc != SUCCESS:
            raise IciktError(f"icikt_multi_create(devices={self.devices}, exchange={exchange!r}) failed with code {rc}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().icikt_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def uses_rccl(self) -> bool:
        return bool(lib().icikt_multi_uses_rccl(self._h))

    def block_bounds(self) -> list:
        """Pair blocks of the last call: rank r ran pairs [b[r], b[r + 1]) of the list."""
        n = self.ranks_used + 1
        b = (ctypes.c_int64 * n)()
        self._chk(lib().icikt_multi_block_bounds(self._h, b), "icikt_multi_block_bounds")
        return list(b)

    @property
    def comm_ranks(self) -> int:
        """Ranks of the RCCL communicator as RCCL reports them (0: device copies, no communicator)."""
        return int(lib().icikt_multi_comm_ranks(self._h))

    def _chk(self, rc: int, what: str):
        if rc != SUCCESS:
            msg = lib().icikt_multi_last_error(self._h)
            raise IciktError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")

    def debug_set_plan(self, spec: str | dict | None = None):
        if isinstance(spec, dict):
            spec = ",".join(f"{k}={v}" for k, v in spec.items() if v not in ("", None))
        self._chk(lib().icikt_multi_debug_set_plan(self._h, (spec or "").encode()), "icikt_multi_debug_set_plan")

    def phase_ms(self) -> dict:
        """Phases of the last call, the maximum over the ranks."""
        ms = (ctypes.c_double * len(MULTI_PHASES))()
        self._chk(lib().icikt_multi_phase_ms(self._h, ms), "icikt_multi_phase_ms")
        return dict(zip(MULTI_PHASES, list(ms)))

    def rank_phase_ms(self) -> list:
        """Per rank: its own phases and the time it waited for the others at the barriers ("wait")."""
        out = []
        for r in range(len(self.devices)):
            ms = (ctypes.c_double * (len(MULTI_PHASES) + 1))()
            self._chk(lib().icikt_multi_rank_phase_ms(self._h, r, ms), "icikt_multi_rank_phase_ms")
            out.append(dict(zip(MULTI_PHASES + ("wait",), list(ms))))
        return out

    @property
    def ranks_used(self) -> int:
        """Ranks the last call really used (1: too small to split, or wide columns: the first device alone)."""
        return int(lib().icikt_multi_ranks_used(self._h))

    def matrix(self, X, global_na=None, pi=None, pj=None, perspective="global", alternative="two.sided",
               continuity=False, flags: int = 0, scale_max=True, diag_good=True, want_keep=True):
        """Same contract as Context.matrix()."""
        return _matrix_call(lib().icikt_matrix_multi_f64, self._h, self._chk, X, global_na, pi, pj, perspective,
                            alternative, continuity, flags, scale_max, diag_good, want_keep)

    def pairs(self, X, pi=None, pj=None, perspective="global", alternative="two.sided", continuity=False,
              flags: int = 0, want_counts: bool = True):
        """Same contract as Context.pairs()."""
        Xf = np.asfortranarray(X, dtype=np.float64)
        if Xf.ndim != 2:
            raise ValueError("X must be 2-D (features x samples)")
        n_feat, n_samp = Xf.shape
        if pi is None:
            P = n_samp * (n_samp - 1) // 2
            pi_a = pj_a = None
        else:
            pi_a = np.ascontiguousarray(pi, dtype=np.int32)
            pj_a = np.ascontiguousarray(pj, dtype=np.int32)
            P = pi_a.shape[0]
        alloc = pinned_empty if (flags & FLAG_HOST_PINNED) else np.empty   # (X is the caller's: pinned by the caller)
        out = alloc((P, 4), dtype=np.float64)
        cnt = alloc((P, len(CNT_FIELDS)), dtype=np.int64) if want_counts else None
        rsn = alloc(P, dtype=np.int32)
        if cnt is not None:
            cnt[...] = 0
        rsn[...] = 0
        alt = ALTERNATIVE.get(alternative, ALT_OTHER)
        self._chk(lib().icikt_pairs_multi_f64(self._h, _ptr(Xf), n_feat, n_samp, max(n_feat, 0), _ptr(pi_a), _ptr(pj_a),
                                              P, PERSPECTIVE[perspective], alt, int(bool(continuity)), flags, _ptr(out),
                                              _ptr(cnt), _ptr(rsn)), "icikt_pairs_multi_f64")
        return out, cnt, rsn


_default_ctx: dict[int, Context] = {}


def default_context(device: int | None = None) -> Context:
    if device is None:
        device = int(os.environ.get("ICIKT_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        n = device_count()
        if n > 0:
            device %= n
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
