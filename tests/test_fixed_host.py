"""The fixed-point quantisation of PERMANOVA's squared dissimilarities (csrc/icikt_fixed.h) against numpy and against
exact rational arithmetic, without a GPU and without the library: tests/fixed_print.cpp is compiled with the host
compiler (with the address and undefined-behaviour sanitizers where they link) and prints what the header makes of the
doubles it reads.  The numpy side is the rule as the front end's fallback states it, `np.rint(np.ldexp(d * d, 50))`; the
rational side rounds `Fraction(d * d) * 2**50` half to even, as tests/permanova_checker.py does."""
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fixed_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def q_numpy(raw):
    d = 1.0 - (np.asarray(raw, dtype=np.float64) + 0.0)
    return np.rint(np.ldexp(d * d, 50)).astype(np.int64)


def q_exact(raw):
    d = 1.0 - (float(raw) + 0.0)
    return round(Fraction(d * d) * 2 ** 50)


def _halves():
    """raw values whose e 2^50 ends in exactly .5: for d in [sqrt 2, 2] the square e lies in [2, 4), where a double's
    last bit is 2^-51, so e 2^50 is a whole number or a whole number and a half"""
    rng = np.random.default_rng(5050)
    raw = rng.uniform(-1.0, -0.42, size=4000)
    d = 1.0 - raw
    e2 = np.ldexp(d * d, 51)
    assert np.all(e2 == np.floor(e2)) and np.all(d * d >= 2.0)
    odd = e2.astype(np.int64) % 2 == 1
    floor_parity = (e2.astype(np.int64) // 2) % 2
    return raw[odd & (floor_parity == 0)], raw[odd & (floor_parity == 1)]


NAMED = np.array([1.0, -1.0, 0.0, -0.0, 1.0 - 2.0 ** -53, np.nan], dtype=np.float64)
RANDOM = np.random.default_rng(2050).uniform(-1.0, 1.0, size=10000)
HALF_DOWN, HALF_UP = _halves()     # ... .5 above an even number (rounds down), above an odd number (rounds up)
VALUES = np.concatenate([NAMED, RANDOM, HALF_DOWN, HALF_UP])


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    prog = str(tmp_path_factory.mktemp("fixed") / "fixed_print")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", prog]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:   # (no sanitizer runtime here)
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    r = subprocess.run([prog], input="".join(f"{int(w)}\n" for w in bits(VALUES)), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_constants(out):
    assert out["frac_bits"] == 50 and out["q_max"] == 2 ** 52 and out["na_key"] == 2 ** 64 - 1
    assert out["limbs"] == [0x89ABCDEF, 0x1234567]
    assert (out["limbs"][1] << 32) + out["limbs"][0] == 0x123456789ABCDEF


def test_named_values(out):
    assert 1.0 - 2.0 ** -53 == np.nextafter(1.0, 0.0)
    assert out["q"][:6] == [0, 2 ** 52, 2 ** 50, 2 ** 50, 0, None]
    assert out["q_key"][:6] == [0, 2 ** 52, 2 ** 50, 2 ** 50, 0, 0]         # NA_KEY adds nothing
    assert out["back"][3] == 0 and out["back"][5] is None                    # -0 comes back as +0


def test_random_values_are_numpys(out):
    lo, hi = len(NAMED), len(NAMED) + len(RANDOM)
    want = q_numpy(RANDOM)
    assert out["q"][lo:hi] == [int(x) for x in want]
    assert out["q_key"][lo:hi] == out["q"][lo:hi]
    assert out["back"][lo:hi] == [int(b) for b in bits(RANDOM)]
    assert want.min() >= 0 and want.max() <= 2 ** 52 and len(set(want.tolist())) > 9000


def test_random_values_are_exact_rationals(out):
    lo = len(NAMED)
    for k in range(0, len(RANDOM), 7):
        assert out["q"][lo + k] == q_exact(RANDOM[k]), RANDOM[k]


def test_halves_round_to_even(out):
    assert len(HALF_DOWN) > 100 and len(HALF_UP) > 100
    at = len(NAMED) + len(RANDOM)
    for values, step in ((HALF_DOWN, 0), (HALF_UP, 1)):
        got = out["q"][at:at + len(values)]
        assert out["q_key"][at:at + len(values)] == got
        assert got == [int(x) for x in q_numpy(values)]
        for raw, q in zip(values, got):
            exact = Fraction((1.0 - raw) * (1.0 - raw)) * 2 ** 50
            assert exact.denominator == 2                         # exactly a half
            assert q == exact.numerator // 2 + step and q % 2 == 0 and q == q_exact(raw)
        at += len(values)
