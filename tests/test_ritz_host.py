"""csrc/icikt_ritz.h without a GPU and without the library: tests/ritz_print.cpp is compiled with the host compiler (with
the address and undefined-behaviour sanitizers where they link) and prints what the header makes of what it reads.

The symmetric eigen-solver (Householder + implicit QL) is held against numpy.linalg.eigh on matrices of order 1, 2, 3,
17 and 128, one family with a repeated eigenvalue: every eigenvalue within FACTOR L eps |H|_F of eigh's, and the
vectors by what defines them, |H Z - Z diag(w)|_max within the same bound and |Z^T Z - I|_max within FACTOR L eps.
FACTOR = 4: measured on the CPU over these cases (g++ -O1, x86-64), in units of L eps max(|H|_F, 1), the largest
eigenvalue error is 0.77 (L = 3, the repeated eigenvalue), the largest residual entry 0.48 (the same matrix) and the
largest departure from orthonormality 0.30 (L = 3, rank 2); at L = 128 all three are below 0.04.  The bound is the
textbook one for a backward-stable symmetric solver, p(L) eps |H|_2 with a modest p; 4 leaves room for another
compiler's rounding of the same operations, not for another algorithm.

The rational-to-double conversion is held against Python's int / int, bit for bit: numerators up to 2^68 (and the
entry's largest, below 2^84), every divisor 2 .. 65 535 (as S 2^50, and as S^2 2^50 for a sample of them), and exact
halves on both sides of an even mantissa."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ritz_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")
FACTOR = 4.0
EPS = 2.0 ** -52
M64 = (1 << 64) - 1


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ritz") / "ritz_print")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:   # (no sanitizer runtime here)
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return exe


def _run(prog, text):
    r = subprocess.run([prog], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _matrices():
    rng = np.random.default_rng(27)
    out = []
    for L in (1, 2, 3, 17, 128):
        A = rng.standard_normal((L, L))
        out.append((f"random{L}", (A + A.T) / 2))
        # a repeated eigenvalue: an orthogonal similarity of a diagonal with the value 2 three times (twice, once)
        Q, _ = np.linalg.qr(rng.standard_normal((L, L)))
        w = rng.uniform(-1.0, 1.0, L)
        w[:min(3, L)] = 2.0
        R = (Q * w) @ Q.T
        out.append((f"repeated{L}", (R + R.T) / 2))
        # a Gram matrix of rank 2 (PCoA's kind: positive semi-definite, most eigenvalues 0), and a diagonal one
        B = rng.standard_normal((L, min(2, L)))
        out.append((f"lowrank{L}", B @ B.T))
        out.append((f"diagonal{L}", np.diag(rng.standard_normal(L))))
    out.append(("zero5", np.zeros((5, 5))))
    return out


def test_eigen_solver_against_eigh(prog):
    cases = _matrices()
    text = "".join(f"e {H.shape[0]}\n" + "".join(f"{int(w)}\n" for w in bits(H).ravel()) for _name, H in cases)
    lines = _run(prog, text)
    assert len(lines) == len(cases)
    worst = {}
    for (name, H), line in zip(cases, lines):
        L = H.shape[0]
        head, *words = line.split()
        assert head == "ok" and len(words) == L + L * L, name
        vals = np.array([int(w) for w in words], dtype=np.uint64).view(np.float64)
        w, Z = vals[:L], vals[L:].reshape(L, L)
        want = np.linalg.eigh(H)[0]
        bound = FACTOR * L * EPS * np.linalg.norm(H)
        figures = (np.abs(w - want).max(), np.abs(H @ Z - Z * w).max(), np.abs(Z.T @ Z - np.eye(L)).max())
        unit = L * EPS * max(np.linalg.norm(H), 1.0)
        print(name, "in units of L eps max(|H|_F, 1):", [float(f / unit) for f in figures])
        worst[L] = np.maximum(worst.get(L, 0.0), np.array(figures) / unit)
        assert np.all(np.diff(w) >= 0), name                                  # ascending
        assert figures[0] <= bound, (name, figures, bound)
        assert figures[1] <= bound, (name, figures, bound)
        assert figures[2] <= FACTOR * L * EPS, (name, figures)
    print({L: [float(x) for x in v] for L, v in worst.items()})


def _ratio_cases():
    rng = np.random.default_rng(68)
    cases = []
    for S in range(2, 65536):                      # every divisor, as the entry forms it: S 2^50
        nb = int(rng.integers(1, 69))
        num = int(rng.integers(0, 1 << 62)) << 6 | int(rng.integers(0, 64))
        num = (num >> (68 - nb)) | (1 << (nb - 1))
        cases.append((num, S << 50))
    for S in rng.integers(2, 65536, 3000):        # m-bar: S^2 2^50 under a sum of up to 2^84
        S = int(S)
        num = (int(rng.integers(0, 1 << 62)) << 22) | int(rng.integers(0, 1 << 22))
        cases.append((num, (S * S) << 50))
    for den in (3, 5, 7, 65535, 65535 * 65535, 12345):   # exact halves: num / den = (2 m + 1) / 2 2^k, m of 53 bits
        for m in (1 << 52, (1 << 52) + 1, (1 << 53) - 1, (1 << 53) - 2, (1 << 52) + 12345):
            for up in (0, 3, 10):
                cases.append((((2 * m + 1) * den) << up, den << 5))           # the tie itself: a 54-bit odd mantissa
                cases.append(((((2 * m + 1) * den) << up) + 1, den << 5))     # a hair above it
                cases.append(((((2 * m + 1) * den) << up) - 1, den << 5))     # a hair below it
    cases += [(0, 7), (1, 1), (1, 3), ((1 << 68), 65535 << 50), ((1 << 68) - 1, 2 << 50), ((1 << 84) - 1, (65535 ** 2) << 50),
              (1 << 52, 65535 << 50), (5, 2), (1 << 60, 1 << 50), ((1 << 53) + 1, 1), ((1 << 54) + 2, 1), ((1 << 54) + 6, 1)]
    return cases


def test_ratio_to_double_is_pythons_division(prog):
    cases = _ratio_cases()
    assert {d >> 50 for _n, d in cases[:65534]} == set(range(2, 65536))
    assert max(n for n, _d in cases[:65534]) >= 1 << 67
    text = "".join(f"r {n >> 64} {n & M64} {d >> 64} {d & M64}\n" for n, d in cases)
    lines = _run(prog, text)
    assert len(lines) == len(cases)
    got = np.array([int(x) for x in lines], dtype=np.uint64)
    want = bits(np.array([n / d for n, d in cases], dtype=np.float64))
    bad = np.flatnonzero(got != want)
    print("cases", len(cases), "differing", bad.size, [cases[i] for i in bad[:5]])
    assert bad.size == 0
