"""The host's key arithmetic (csrc/icikt_keys.h: cor_key and its inverse, max_taumax_of, the two constants) against
numpy, without a GPU and without the library: tests/keys_print.cpp is compiled with the host compiler (with the address
and undefined-behaviour sanitizers where they link) and prints what the header makes of the words on its command line.
The numpy side states the two encodings from the device's definitions: colsort::cor_key (csrc/icikt_colsort.h) and
dbl_sortable (csrc/icikt_epilogue.hip)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "keys_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")

TOP = np.uint64(1) << np.uint64(63)
NA_KEY = 2 ** 64 - 1                  # colsort::NA_KEY = ~0ull
R_NA_BITS = 0x7FF00000000007A2        # R's NA_real_: a NaN whose low word is 1954


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def cor_key(v):
    """__device__ cor_key: `if (v != v) return NA_KEY; if (v == 0.0) v = 0.0; b = bits(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));`"""
    v = np.array(v, dtype=np.float64)
    v[v == 0.0] = 0.0
    b = bits(v)
    k = np.where(b >> np.uint64(63) != 0, ~b, b | TOP)
    return np.where(v != v, np.uint64(NA_KEY), k)


def dbl_sortable(v):
    """__device__ dbl_sortable: `u = bits(v); return (u >> 63) ? ~u : (u | 0x8000000000000000ull);` -- -0.0 keeps its sign"""
    u = bits(v)
    return np.where(u >> np.uint64(63) != 0, ~u, u | TOP)


def _values():
    tiny, big = 5e-324, np.finfo(np.float64).max
    named = np.array([0.0, -0.0, tiny, -tiny, 1.0, -1.0, big, -big, np.inf, -np.inf, np.nan], dtype=np.float64)
    rng = np.random.default_rng(20260)
    words = rng.integers(0, 2 ** 64, size=200, dtype=np.uint64).view(np.float64)     # any bit pattern, NaNs among them
    taus = rng.uniform(-1.0, 1.0, size=100)                                           # what the planes hold
    wide = rng.standard_normal(100) * 10.0 ** rng.integers(-300, 300, size=100)
    near = np.nextafter(np.array([0.0, 1.0, -1.0, 0.5]), np.array([1.0, 2.0, -2.0, 0.0]))
    r_na = np.array([R_NA_BITS, R_NA_BITS | (1 << 63)], dtype=np.uint64).view(np.float64)
    return np.concatenate([named, r_na, words, taus, wide, near, -near])


VALUES = _values()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("keys") / "keys_print")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:   # (no sanitizer runtime here)
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr

    def run(mode, words):
        r = subprocess.run([out, mode, *(str(int(w)) for w in words)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    return run


@pytest.fixture(scope="module")
def cor(prog):
    return prog("cor", bits(VALUES))


def test_constants(cor):
    assert cor["na_key"] == NA_KEY and cor["r_na_bits"] == R_NA_BITS
    assert np.isnan(np.array([R_NA_BITS], dtype=np.uint64).view(np.float64)[0])


def test_cor_key_is_the_devices(cor):
    assert cor["key"] == [int(k) for k in cor_key(VALUES)]


def test_key_order_is_value_order(cor):
    valid = ~np.isnan(VALUES)
    assert valid.sum() > 300
    v = VALUES[valid]
    k = np.array([cor["key"][i] for i in np.nonzero(valid)[0]], dtype=np.uint64)
    order = np.argsort(v, kind="stable")
    v, k = v[order], k[order]
    assert np.array_equal(v[1:] > v[:-1], k[1:] > k[:-1])
    assert np.array_equal(v[1:] == v[:-1], k[1:] == k[:-1])
    assert (v[1:] > v[:-1]).sum() > 300                # (not a comparison of equal values only)
    assert int(k.max()) < NA_KEY and int(k.min()) > 0   # NA_KEY is above every value, 0 below


def test_zeros_share_a_key_and_come_back_positive(cor):
    plus, minus = 0, 1
    assert VALUES[plus] == 0.0 and not np.signbit(VALUES[plus]) and VALUES[minus] == 0.0 and np.signbit(VALUES[minus])
    assert cor["key"][plus] == cor["key"][minus] == 1 << 63
    assert cor["back"][plus] == cor["back"][minus] == 0


def test_nan_is_na_key(cor):
    nan = np.nonzero(np.isnan(VALUES))[0]
    assert len(nan) >= 3                                # NaN, NA_real_ and its negative at least
    for i in nan:
        assert cor["key"][i] == NA_KEY and cor["back"][i] is None


def test_inverse_round_trips(cor):
    b = bits(VALUES)
    n = 0
    for i, v in enumerate(VALUES):
        if np.isnan(v) or (v == 0.0 and np.signbit(v)):
            continue
        assert cor["back"][i] == int(b[i]), (i, v)
        n += 1
    assert n > 300


def test_max_taumax_of(prog):
    finite = VALUES[np.isfinite(VALUES)]
    assert np.signbit(finite[1]) and finite[1] == 0.0   # -0.0 is among them
    words = dbl_sortable(finite)
    assert int(words[0]) != int(words[1])               # the plain order keeps -0.0 apart from +0.0
    assert all(int(w) != 0 for w in words)              # 0 is no double's word
    got = prog("taumax", [0, *words])["bits"]
    assert got[0] == int(bits(-np.inf))                 # no pair had a taumax: max(numeric(0), na.rm = TRUE)
    assert got[1:] == [int(x) for x in bits(finite)]
