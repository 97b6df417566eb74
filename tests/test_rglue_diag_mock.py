"""The R glue of the missing-value diagnostics (icikendalltau_amd/r/icikt_rglue_diag.c) compiled WITHOUT R against the
test double of tests/r_mock (with warnings as errors) and driven through the mock's .Call: registration, arities and
argument checks on the CPU, the results against the Python binding of the same C ABI under -m gpu."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_rglue_mock import MOCK, R, ROOT, _call_arity

GLUE = os.path.join(ROOT, "icikendalltau_amd", "r", "icikt_rglue.c")
GLUE_DIAG = os.path.join(ROOT, "icikendalltau_amd", "r", "icikt_rglue_diag.c")
RWRAP = os.path.join(ROOT, "icikendalltau_amd", "r", "icikt_mi355x.R")
OUT = os.path.join(MOCK, "_build", "librglue_diag_mock.so")
ROUTINES = {"icikt_R_col_medians": 4, "icikt_R_censor_counts": 4, "icikt_R_rank_order": 4}


class DllInfo(ctypes.Structure):
    _fields_ = [("dynamic_symbols", ctypes.c_int)]


@pytest.fixture(scope="module")
def glue():
    from icikendalltau_amd import _lib
    if _lib.needs_build():
        _lib.build()
    _lib.lib()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Wno-cast-function-type", "-Werror", "-fPIC", "-shared",
           "-I", MOCK, "-I", os.path.join(ROOT, "include"), GLUE, GLUE_DIAG, os.path.join(MOCK, "r_mock.c"),
           "-L", libdir, "-licikt_hip", f"-Wl,-rpath,{libdir}", "-o", OUT]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = ctypes.CDLL(OUT)
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    for name, res, args in [("mock_null", vp, []), ("mock_real_vector", vp, [vp, cl]), ("mock_real_matrix", vp, [vp, ci, ci]),
                            ("mock_int_vector", vp, [vp, cl]), ("mock_logical", vp, [ci]), ("mock_string", vp, [ctypes.c_char_p]),
                            ("mock_type", ci, [vp]), ("mock_length", cl, [vp]), ("mock_is_matrix", ci, [vp]),
                            ("mock_nrow", ci, [vp]), ("mock_ncol", ci, [vp]), ("mock_data", vp, [vp]),
                            ("mock_list_elt", vp, [vp, cl]), ("mock_list_name", ctypes.c_char_p, [vp, cl]),
                            ("mock_dotcall", vp, [ctypes.c_char_p, ci, ctypes.POINTER(vp)]),
                            ("mock_last_error", ctypes.c_char_p, []), ("mock_routine_name", ctypes.c_char_p, [ci]),
                            ("mock_routine_nargs", ci, [ci]), ("mock_n_routines", ci, []), ("mock_protect_depth", ci, []),
                            ("mock_reset", None, [])]:
        getattr(L, name).restype = res
        getattr(L, name).argtypes = args
    dll = DllInfo(1)
    L.R_init_icikt_rglue_diag(ctypes.byref(dll))
    L.dll = dll
    yield L
    L.R_unload_icikt_rglue_diag(ctypes.byref(dll))
    L.mock_reset()


def test_diag_glue_registers_and_checks_arguments(glue):
    L, r = glue, R(glue)
    table = {L.mock_routine_name(i).decode(): L.mock_routine_nargs(i) for i in range(L.mock_n_routines())}
    assert table == ROUTINES
    assert L.dll.dynamic_symbols == 0
    wrapper = open(RWRAP).read()
    for name, nargs in ROUTINES.items():
        assert _call_arity(wrapper, name) == nargs   # the R wrappers call them with their registered arity
    for fn in ("calculate_matrix_medians_gpu", "test_left_censorship_gpu", "rank_order_data_gpu"):
        assert f"{fn} = function(" in wrapper
    with pytest.raises(RuntimeError, match="x must be a double matrix"):
        r.call("icikt_R_col_medians", r.real([1.0]), r.null, r.lgl(0), r.int1(0))
    X = r.matrix(np.zeros((4, 3)))
    gna = r.real([math.nan, math.inf, 0.0])
    with pytest.raises(RuntimeError, match="one class per column"):
        r.call("icikt_R_censor_counts", X, gna, r.ints([1, 1]), r.int1(0))
    with pytest.raises(RuntimeError, match="class index out of range"):
        r.call("icikt_R_censor_counts", X, gna, r.ints([1, 0, 3]), r.int1(0))
    with pytest.raises(RuntimeError, match="global_na must be a double vector"):
        r.call("icikt_R_censor_counts", X, r.chr("NA"), r.ints([1, 1, 1]), r.int1(0))
    with pytest.raises(RuntimeError, match="column index out of range"):
        r.call("icikt_R_rank_order", X, gna, r.ints([1, 4]), r.int1(0))


@pytest.mark.gpu
def test_diag_glue_matches_the_binding(glue):
    from icikendalltau_amd import _lib
    r = R(glue)
    ctx = _lib.default_context(0)
    rng = np.random.default_rng(5)
    X = rng.lognormal(2, 1, size=(300, 6))
    X[rng.random(X.shape) < 0.2] = np.nan
    X[rng.random(X.shape) < 0.05] = 0.0
    X[7, :3] = np.nan
    gna = [math.nan, math.inf, 0.0]
    med = r.value(r.call("icikt_R_col_medians", r.matrix(X), r.null, r.lgl(1), r.int1(0)))
    np.testing.assert_array_equal(med.view(np.uint64), ctx.col_medians(X, True).view(np.uint64))
    cls = np.array([2, 1, 2, 1, 1, 2], np.int32)
    got = r.value(r.call("icikt_R_censor_counts", r.matrix(X), r.real(gna), r.ints(cls), r.int1(0)))
    tr, su, nex, _ = ctx.censor_counts(X, gna, cls - 1, 2)
    np.testing.assert_array_equal(got["trials"], tr)
    np.testing.assert_array_equal(got["success"], su)
    assert got["n_excluded"][0] == nex
    cols = np.array([1, 3, 4], np.int32)
    got = r.value(r.call("icikt_R_rank_order", r.matrix(X), r.real(gna), r.ints(cols), r.int1(0)))
    ref = ctx.rank_order(X, gna, cols - 1)
    kept = ref["n_na"] < 3
    np.testing.assert_array_equal(got["n_na"], ref["n_na"][kept])
    np.testing.assert_array_equal(got["median_rank"], ref["median_rank"][kept])
    np.testing.assert_array_equal(got["row_order"], ref["row_order"] + 1)
    np.testing.assert_array_equal(got["col_order"], ref["col_order"] + 1)
    np.testing.assert_array_equal(got["original"].view(np.uint64), ref["original"].view(np.uint64))
    np.testing.assert_array_equal(got["ordered"].view(np.uint64), ref["ordered"].view(np.uint64))
