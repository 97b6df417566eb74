"""What oracle/rcpp_standin/Rcpp.h CLAIMS Rcpp does, stated against numpy on the edges that matter to the reference's
src/kendallc.cpp -- without a GPU, without the library and without the reference: tests/rcpp_standin_print.cpp is
compiled by the host compiler under -Wall -Wextra -Werror (with the address and undefined-behaviour sanitizers where
they link: the stand-in promises to wrap without undefined behaviour) and prints what the header makes of the numbers
on its command line.  Rcpp itself is not available, so these claims are a READING of its documented behaviour
(DESIGN.md section 6 lists them); the compiled reference (tests/test_oracle_vs_reference.py) stands on them."""
import json
import os
import subprocess

import mpmath
import numpy as np
import pytest

from tests import epilogue_checker as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "rcpp_standin_print.cpp")
STANDIN = os.path.join(ROOT, "oracle", "rcpp_standin")

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
NA_INTEGER = INT_MIN
R_NA_BITS = 0x7FF00000000007A2


def bits(v):
    return [int(w) for w in np.atleast_1d(np.asarray(v, dtype=np.float64)).view(np.uint64)]


def doubles(words):
    return np.array(words, dtype=np.uint64).view(np.float64)


def wrap(v):
    """A Python integer as the int32 it wraps to."""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def na_or(f, *args):
    return NA_INTEGER if NA_INTEGER in args else wrap(f(*args))


def trunc_div(a, b):
    """C's a / b for b > 0: toward zero; NA_INTEGER stays."""
    return NA_INTEGER if a == NA_INTEGER else -(-a // b) if a < 0 else a // b


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rcpp_standin") / "rcpp_standin_print")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", STANDIN, SRC,
            "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:   # (no sanitizer runtime here)
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr

    def run(mode, *lists):
        args = []
        for k, lst in enumerate(lists):
            args += (["--"] if k else []) + [str(int(v)) for v in lst]
        r = subprocess.run([out, mode, *args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    return run


A = [INT_MAX, INT_MAX, 46341, 65536, -7, 7, NA_INTEGER, 3, 0, -5, 1100, 1300, 46400, 3, 3]
B = [1, INT_MAX, 46341, 65536, 2, -2, 5, NA_INTEGER, 0, -5, 1099, 1299, 46399, 2, 1]
S = 2


@pytest.fixture(scope="module")
def ints(prog):
    return prog("int", A, B, [S])


def test_int_arithmetic_wraps_and_propagates_na(ints):
    """int wrap at INT_MAX (INT_MAX + 1 = INT_MIN + 0 ... the wrapped value, which for + 1 is NA_INTEGER's own pattern),
    products past 2^31 and 2^32, NA_INTEGER through + - * and /."""
    assert ints["add"] == [na_or(lambda a, b: a + b, a, b) for a, b in zip(A, B)]
    assert ints["sub"] == [na_or(lambda a, b: a - b, a, b) for a, b in zip(A, B)]
    assert ints["mul"] == [na_or(lambda a, b: a * b, a, b) for a, b in zip(A, B)]
    assert ints["add_s"] == [na_or(lambda a: a + S, a) for a in A]
    assert ints["sub_s"] == [na_or(lambda a: a - S, a) for a in A]
    assert ints["s_sub"] == [na_or(lambda a: S - a, a) for a in A]
    assert ints["mul_s"] == ints["s_mul"] == [na_or(lambda a: a * S, a) for a in A]
    assert ints["add"][0] == INT_MIN and ints["add"][1] == -2 and ints["mul"][2] == wrap(46341 ** 2) < 0
    assert ints["mul"][3] == 0                                      # 2^32 wraps to 0
    assert ints["mul"][6] == ints["mul"][7] == ints["sub"][6] == NA_INTEGER


def test_int_division_truncates_toward_zero(ints):
    assert ints["div_s"] == [trunc_div(a, S) for a in A]
    assert ints["div_s"][4] == -3 and ints["div_s"][9] == -2        # -7 / 2 and -5 / 2: not floor's -4 and -3
    assert ints["div_s"][6] == NA_INTEGER


def test_int_sum_propagates_na_and_wraps(ints, prog):
    assert ints["sum"] == NA_INTEGER and ints["sum_half"] == NA_INTEGER
    vals = [INT_MAX, INT_MAX, 5, -3]
    got = prog("int", vals, vals, [S])
    assert got["sum"] == wrap(sum(vals)) == 0
    vals = [INT_MAX, 10]                                            # wraps to a negative sum; its half truncates
    got = prog("int", vals, vals, [S])
    assert got["sum"] == wrap(sum(vals)) == INT_MIN + 9 and got["sum_half"] == trunc_div(INT_MIN + 9, 2) == -1073741819
    assert got["sum_half"] != (INT_MIN + 9) // 2                    # floor would differ


@pytest.mark.parametrize("sizes", [[2, 3, 5], [1100], [1300, 2], [46400, 7], [1100, 1100, 1300], [46341, 46341]])
def test_the_tie_sums_of_count_rank_tie_wrap_in_int(prog, sizes):
    """The three expressions of kendallc.cpp:112-114 on group sizes on either side of each wrap: every element product
    and the running sum are int32, and `/ 2` truncates the wrapped sum."""
    got = prog("int", sizes, sizes, [S])
    tt1 = wrap(sum(wrap(t * (t - 1)) for t in sizes))
    assert got["tt1"] == tt1 and got["tt1_half"] == trunc_div(tt1, 2)
    assert got["t0"] == wrap(sum(wrap(wrap(t * (t - 1)) * (t - 2)) for t in sizes))
    assert got["t1"] == wrap(sum(wrap(wrap(t * (t - 1)) * wrap(2 * t + 5)) for t in sizes))
    exact = sum(t * (t - 1) * (2 * t + 5) for t in sizes)
    assert (got["t1"] != exact) == (max(sizes) >= 1100)


def test_cumsum_diff_max_seq_along(ints, prog):
    vals = [1, 0, 0, 1, 1, 0, 1]
    got = prog("int", vals, vals, [S])
    assert got["cumsum"] == np.cumsum(vals).tolist() and got["diff"] == np.diff(vals).tolist()
    assert got["seq_along"] == list(range(1, len(vals) + 1)) and got["max"] == 1
    assert ints["cumsum"][:6] == [wrap(v) for v in np.cumsum(np.array(A[:6], dtype=object))]
    assert ints["cumsum"][6:] == [NA_INTEGER] * (len(A) - 6)        # NA from its position on
    assert ints["diff"][0] == 0 and ints["diff"][5] == ints["diff"][6] == NA_INTEGER
    assert prog("int", [5], [5], [S])["diff"] == []


def test_table_and_duplicated_of_integers(prog):
    vals = [3, -1, 3, 7, -1, 3, 0, 7, 12]
    got = prog("int", vals, vals, [S])
    keys, counts = np.unique(vals, return_counts=True)
    assert got["table"] == counts.tolist() and keys.tolist() == sorted(set(vals))      # in ascending key order
    first = [vals.index(v) == i for i, v in enumerate(vals)]
    assert got["duplicated"] == [0 if f else 1 for f in first]                          # the first occurrence is not
    assert got["which_dup"] == [v for v, f in zip(vals, first) if not f]


X = np.array([1.5, -0.0, np.nan, 0.0, 2.5, 1.5, -3.0, 0.0, np.inf, -np.inf, 5e-324, 1.5])
X_WORDS = bits(X)
X_WORDS[7] = R_NA_BITS                                                # NA_real_ beside the plain NaN
X = doubles(X_WORDS)
AT = [4, 0, 0, 11, 6]
KEEP = [1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1]


@pytest.fixture(scope="module")
def real(prog):
    return prog("real", X_WORDS, AT, KEEP)


def test_is_na_is_true_for_nan_and_na_real(real):
    assert np.isnan(X[2]) and np.isnan(X[7]) and X_WORDS[2] != X_WORDS[7]
    assert real["is_na"] == [1 if i in (2, 7) else 0 for i in range(len(X))] and real["n_na"] == 2
    assert real["na_omit"] == [w for i, w in enumerate(X_WORDS) if i not in (2, 7)]


def test_table_unique_duplicated_of_doubles_take_the_zeros_as_one_key(real):
    v = X[~np.isnan(X)]
    keys, counts = np.unique(v, return_counts=True)                  # numpy: -0.0 == 0.0, ascending
    assert real["table"] == counts.tolist() and counts[keys == 0.0].tolist() == [2]
    first = [next(j for j, u in enumerate(v) if u == w) == i for i, w in enumerate(v)]
    assert real["duplicated"] == [0 if f else 1 for f in first]
    assert real["duplicated"][2] == 1                                # +0.0 after -0.0 is a duplicate
    assert doubles(real["unique"]).tolist() == [w for w, f in zip(v, first) if f]


def test_subsetting_and_logical_index_assignment(real):
    assert real["by_int"] == [X_WORDS[i] for i in AT]
    assert real["by_lgl"] == [w for w, k in zip(X_WORDS, KEEP) if k]
    assert real["by_not"] == [w for w, k in zip(X_WORDS, KEEP) if not k]
    assert real["assigned"] == [bits(7.5)[0] if k else w for w, k in zip(X_WORDS, KEEP)]
    assert real["untouched"] == X_WORDS                              # clone() copied: value semantics
    nan = np.isnan(X)
    assert real["and"] == [int(k and m) for k, m in zip(KEEP, nan)] and real["or"] == [int(k or m) for k, m in zip(KEEP, nan)]
    assert doubles(real["from_int"]).tolist() == [float(i) for i in AT]


def test_double_arithmetic_and_reductions(real):
    v = X[~np.isnan(X)]
    assert real["plus"] == bits(v + 0.1) and real["minus"] == bits(v - 0.1)
    assert real["times"] == bits(2.0 * v) and real["over"] == bits(v / 3.0)
    assert doubles(real["min"])[0] == -np.inf and np.isnan(doubles(real["sum"])[0])   # inf + -inf


def test_sum_of_doubles_accumulates_left_to_right_in_double(prog):
    w = np.array([0.1] * 10 + [1e16, 1.0, -1e16])
    acc = 0.0
    for u in w:
        acc += u
    got = prog("real", bits(w), [0], [0] * len(w))
    assert got["sum"] == bits(acc) and acc != float(mpmath.fsum([float(u) for u in w]))
    assert doubles(got["min"])[0] == -1e16


def test_misc(prog):
    m = prog("misc")
    assert m["na_real"] == [R_NA_BITS] and m["na_integer"] == INT_MIN
    assert m["seq"] == [0, 1, 2, 3, 4] and m["seq_one"] == [3]
    assert m["seq_empty_throws"] == 1                                # seq(0, -1): which_notzero on all zeros would throw
    assert m["stop_throws"] == 1 and m["warnings"] == 2 and m["last_warning_is_second"] == 1
    assert m["captured_ok"] == 1
    assert m["sized"] == [0, 0, 0] and m["zeros"] == bits([0.0] * 4) and m["names"] == 2
    assert m["double_index"] == bits([2.5, 3.5]) and m["string_eq"] == 1


def _grid():
    """The pnorm grid of tests/test_epilogue_reference.py: 3 001 even steps over +-37.5, the three branch edges and
    2^-53 with their neighbours, the zeros, the cut-off's far side and the infinities."""
    z = list(np.linspace(-37.5, 37.5, 3001))
    for e in E.EDGES + (2.0 ** -53,):
        for s in (e, -e):
            z += [np.nextafter(s, -np.inf), s, np.nextafter(s, np.inf)]
    z += [0.0, -0.0, 1e-17, -1e-17, 37.52, -37.52, 40.0, -40.0, np.inf, -np.inf]
    return [float(v) for v in z]


def test_pnorm_against_mpmath(prog):
    """The stand-in's pnorm (erfcl in long double, R's cut-off) on the oracle's grid at the oracle's own bar, 2 E_CPU
    scaled units; it is the better-rounded side (at most about half a unit of the double it returns)."""
    z = _grid()
    got = prog("pnorm", bits(z) + [bits(np.nan)[0]])
    assert got["lower"] == got["lower_explicit"] and got["upper"] == got["upper_explicit"]
    bound = 2 * E.E_CPU["grid"]
    worst = 0.0
    for name, lower_tail in (("lower", True), ("upper", False)):
        p = doubles(got[name])
        assert np.isnan(p[-1])
        for zk, pk in zip(z, p[:-1]):
            want = E.exact_pnorm(zk, lower_tail)
            if abs(zk) >= E.CUTOFF:
                assert pk == float(want) and want in (0, 1), (zk, pk)
            elif want >= E.TINY:
                e = E.scaled_error(pk, want, zk)
                worst = max(worst, e)
                assert e <= bound, (zk, pk, float(want), e)
            else:
                assert abs(pk - want) <= bound * (1 + zk * zk) * E.UNIT * want + 4 * 2.0 ** -1074, (zk, pk)
    print(f"\nstand-in pnorm: worst scaled error {worst:.3f} (bar {bound})")
    assert doubles(got["lower"])[z.index(0.0)] == 0.5 and doubles(got["upper"])[z.index(0.0)] == 0.5
