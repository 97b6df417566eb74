"""The R glue of cor_fast (icikendalltau_amd/r/icikt_rglue_cor.c) compiled WITHOUT R against the test double of
tests/r_mock (with warnings as errors) and driven through the mock's .Call: registration and arity on the CPU, the
results against the Python binding of the same C ABI under -m gpu."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.test_rglue_mock import MOCK, R, ROOT, _call_arity

GLUE = os.path.join(ROOT, "icikendalltau_amd", "r", "icikt_rglue.c")
GLUE_COR = os.path.join(ROOT, "icikendalltau_amd", "r", "icikt_rglue_cor.c")
RWRAP = os.path.join(ROOT, "icikendalltau_amd", "r", "icikt_mi355x.R")
OUT = os.path.join(MOCK, "_build", "librglue_cor_mock.so")


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
    # r_mock.c's driver initialises icikt_rglue.c: both glue files go in, the cor table is registered below
    cmd = ["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Wno-cast-function-type", "-Werror", "-fPIC", "-shared",
           "-I", MOCK, "-I", os.path.join(ROOT, "include"), GLUE, GLUE_COR, os.path.join(MOCK, "r_mock.c"),
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
    L.R_init_icikt_rglue_cor(ctypes.byref(dll))
    L.dll = dll
    yield L
    L.R_unload_icikt_rglue_cor(ctypes.byref(dll))
    L.mock_reset()


def test_cor_glue_registers_and_checks_arguments(glue):
    L, r = glue, R(glue)
    table = {L.mock_routine_name(i).decode(): L.mock_routine_nargs(i) for i in range(L.mock_n_routines())}
    assert table == {"icikt_R_cor": 9}
    assert L.dll.dynamic_symbols == 0
    wrapper = open(RWRAP).read()
    assert _call_arity(wrapper, "icikt_R_cor") == 9    # the R wrapper calls it with its registered arity
    args = [r.real([1.0, 2.0]), r.ints([1]), r.ints([2]), r.chr("pearson"), r.lgl(0), r.chr("two.sided"), r.lgl(0),
            r.int1(0), r.lgl(0)]
    with pytest.raises(RuntimeError, match="x must be a double matrix"):
        r.call("icikt_R_cor", *args)
    X = r.matrix(np.zeros((4, 2)))
    with pytest.raises(RuntimeError, match="method must be"):
        r.call("icikt_R_cor", X, *args[1:3], r.chr("kendall"), *args[4:])
    with pytest.raises(RuntimeError, match="alternative must be"):
        r.call("icikt_R_cor", X, *args[1:5], r.chr("two-sided"), *args[6:])


@pytest.mark.gpu
def test_cor_glue_matches_the_binding(glue):
    from icikendalltau_amd import _lib
    r = R(glue)
    rng = np.random.default_rng(3)
    X = rng.normal(size=(50, 4))
    X[rng.random(X.shape) < 0.1] = np.nan
    pi, pj = np.array([0, 0, 1, 3], np.int32), np.array([1, 2, 3, 3], np.int32)
    got = r.value(r.call("icikt_R_cor", r.matrix(X), r.ints(pi + 1), r.ints(pj + 1), r.chr("spearman"), r.lgl(1),
                         r.chr("less"), r.lgl(0), r.int1(0), r.lgl(1)))
    out, rsn = _lib.default_context(0).cor_pairs(X, pi, pj, "spearman", True, "less")
    np.testing.assert_array_equal(got["rho"], out[:, 0])
    np.testing.assert_array_equal(got["pvalue"], out[:, 1])
    np.testing.assert_array_equal(got["n_values"], out[:, 2])
    np.testing.assert_array_equal(got["reason"], rsn)
    assert got["kernel_ms"].shape == (3,) and (got["kernel_ms"] >= 0).all()
