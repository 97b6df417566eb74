"""_lib.input_view: which matrices the *_in entries read where they lie (icikt_input: dtype, order, leading dimension)
and which are copied to an F-ordered float64 array first.  No GPU."""
import os
import re

import numpy as np
import pytest

from icikendalltau_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [(np.float64, _lib.DTYPE_F64), (np.float32, _lib.DTYPE_F32), (np.int32, _lib.DTYPE_I32),
          (np.int64, _lib.DTYPE_I64)]
NEW = ("icikt_pairs_in", "icikt_matrix_in", "icikt_pairs_complete_in", "icikt_missingness_in", "icikt_cor_pairs_in",
       "icikt_col_medians_in", "icikt_censor_counts_in", "icikt_rank_order_in", "icikt_convert_dev")


def cell(a, code, order, ld, r, c):
    """element (r, c) as the C side addresses it: data[r + c * ld] (COL) or data[r * ld + c] (ROW)"""
    off = (r + c * ld) if order == _lib.ORDER_COL else (r * ld + c)
    flat = np.lib.stride_tricks.as_strided(a, shape=(off + 1,), strides=(a.dtype.itemsize,), writeable=False)
    return flat[off]


def assert_view(X, code, order, ld):
    a, got_code, got_order, got_ld, copied = _lib.input_view(X)
    assert copied is False and np.shares_memory(a, X) and a.ctypes.data == X.ctypes.data
    assert (got_code, got_order, got_ld) == (code, order, ld)
    for r in range(X.shape[0]):
        for c in range(X.shape[1]):
            assert cell(a, got_code, got_order, got_ld, r, c) == X[r, c]


@pytest.mark.parametrize("dt,code", DTYPES)
@pytest.mark.parametrize("order", ["C", "F"])
def test_contiguous_arrays_pass_without_a_copy(dt, code, order):
    X = np.array(np.arange(15).reshape(5, 3), dtype=dt, order=order)
    assert_view(X, code, _lib.ORDER_ROW if order == "C" else _lib.ORDER_COL, 3 if order == "C" else 5)


@pytest.mark.parametrize("dt,code", DTYPES)
def test_slices_of_contiguous_arrays_pass_with_the_parents_leading_dimension(dt, code):
    C = np.array(np.arange(30).reshape(5, 6), dtype=dt, order="C")
    F = np.array(np.arange(30).reshape(5, 6), dtype=dt, order="F")
    assert_view(C[:, 1:3], code, _lib.ORDER_ROW, 6)     # ld above the extent (2)
    assert_view(C[1:4, :], code, _lib.ORDER_ROW, 6)
    assert_view(F[:, 1:3], code, _lib.ORDER_COL, 5)
    assert_view(F[1:4, :], code, _lib.ORDER_COL, 5)     # ld above the extent (3)


@pytest.mark.parametrize("dt,code", DTYPES)
def test_single_row_and_single_column(dt, code):
    """An extent of 1 leaves one stride unused: the view is read column-major when that fits (ld = n_feat), else
    row-major; either way every cell is addressed where it lies (assert_view checks each)."""
    for order in "CF":
        assert_view(np.array(np.arange(7).reshape(1, 7), dtype=dt, order=order), code, _lib.ORDER_COL, 1)
        assert_view(np.array(np.arange(7).reshape(7, 1), dtype=dt, order=order), code, _lib.ORDER_COL, 7)
    C = np.array(np.arange(30).reshape(5, 6), dtype=dt, order="C")
    assert_view(C[:, 2:3], code, _lib.ORDER_ROW, 6)     # a column of a row-major parent: stride 6 between its cells
    assert_view(C[2:3, :], code, _lib.ORDER_COL, 1)
    F = np.asfortranarray(C)
    assert_view(F[:, 2:3], code, _lib.ORDER_COL, 5)
    assert_view(F[2:3, :], code, _lib.ORDER_COL, 5)     # a row of a column-major parent: stride 5 between its cells


def test_everything_else_is_copied_to_fortran_float64():
    base = np.arange(30, dtype=np.float64).reshape(5, 6)
    F = np.asfortranarray(base)
    cases = {
        "float16": base.astype(np.float16), "uint8": base.astype(np.uint8), "bool": base > 3,
        "X[::2] (both strides non-unit)": F[::2], "X[:, ::2] (both strides non-unit)": base[:, ::2],
        "X[:, ::-1]": base[:, ::-1], "F[::-1]": F[::-1],
        "byte-swapped": base.astype(base.dtype.newbyteorder()), "list of lists": base.tolist(),
        "empty": np.empty((0, 4)), "int16": base.astype(np.int16), "uint32": base.astype(np.uint32),
    }
    for label, X in cases.items():
        a, code, order, ld, copied = _lib.input_view(X)
        assert copied is True, label
        assert a.dtype == np.float64 and a.flags.f_contiguous and a.ndim == 2, label
        assert (code, order, ld) == (_lib.DTYPE_F64, _lib.ORDER_COL, max(a.shape[0], 1)), label
        assert np.array_equal(a, np.asarray(X, dtype=np.float64)), label
    with pytest.raises(ValueError):
        _lib.input_view(np.arange(4.0))


def test_a_copy_clears_the_callers_pinned_flag():
    X = np.arange(12, dtype=np.float32).reshape(4, 3)
    _a, _v, n, S, flags = _lib._view_arg(X, _lib.FLAG_HOST_PINNED | _lib.FLAG_TIMING)
    assert (n, S) == (4, 3) and flags == _lib.FLAG_HOST_PINNED | _lib.FLAG_TIMING
    _a, v, n, S, flags = _lib._view_arg(X.astype(np.float16), _lib.FLAG_HOST_PINNED | _lib.FLAG_TIMING)
    assert flags == _lib.FLAG_TIMING and (v.dtype, v.order, v.ld) == (_lib.DTYPE_F64, _lib.ORDER_COL, 4)


def test_header_declares_the_view_and_the_new_entries():
    src = open(os.path.join(ROOT, "include", "icikt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _lib.EXPORTS, name
    defs = dict(re.findall(r"#define\s+(ICIKT_[A-Z0-9_]+)\s+(\d+)", src))
    assert [int(defs["ICIKT_DTYPE_" + k]) for k in ("F64", "F32", "I32", "I64")] == [
        _lib.DTYPE_F64, _lib.DTYPE_F32, _lib.DTYPE_I32, _lib.DTYPE_I64] == [0, 1, 2, 3]
    assert (int(defs["ICIKT_ORDER_COL"]), int(defs["ICIKT_ORDER_ROW"])) == (_lib.ORDER_COL, _lib.ORDER_ROW) == (0, 1)
    assert re.search(r"typedef\s+struct\s*\{\s*const\s+void\s*\*\s*data;\s*int\s+dtype;\s*int\s+order;\s*int64_t\s+ld;\s*\}\s*icikt_input;", code)
    assert int(defs["ICIKT_VERSION"]) == 400
    import ctypes
    assert ctypes.sizeof(_lib.InputView) == 24 and _lib.InputView.ld.offset == 16
