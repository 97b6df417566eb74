"""ici_kendalltau_pcoa without a device: designed raw matrices go to the brute-force checker
(tests/pcoa_checker.py) and, through an engine whose `pcoa` is api._pcoa_numpy on that raw matrix, to the front end.
What is pinned: the refusals by name, the NA route, the sign rule, total_inertia and the other derived outputs, the
numpy route's integers and centred table against the checker bit for bit, and the checker itself against Fraction
arithmetic on five points of a line worked by hand."""
import os
import re
import warnings
from fractions import Fraction

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests import pcoa_checker as pc
from tests.numpy_ctx import NumpyCtx
from tests.pcoa_checker import bits, na_real

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["coordinates", "eigenvalues", "proportion", "vectors", "total_inertia", "n_positive", "residuals", "frobenius",
        "min_ritz", "n_basis", "n_apply", "converged", "n_valid", "n_na", "sums", "sample_id", "max_taumax", "run_time"]
FLOATS = ("coordinates", "eigenvalues", "proportion", "vectors", "total_inertia", "residuals", "frobenius", "min_ritz")


class RawEngine(NumpyCtx):
    """the numpy engine with the one method this entry looks for: the rule applied to a designed raw matrix"""

    def __init__(self, raw):
        self.raw = np.asarray(raw, dtype=np.float64)
        self.calls = []

    def pcoa(self, X, k, tol, max_basis, seed, return_gower, global_na=None, perspective="global",
             alternative="two.sided", continuity=False, flags=0):
        assert X.shape[1] == self.raw.shape[0]
        self.calls.append((k, tol, max_basis, seed, return_gower))
        out = api._pcoa_numpy(self.raw, k)
        return (*out[:-1], out[-1] if return_gower else None, 0.5, np.zeros(5, dtype=np.int64))


def _front(raw, **kw):
    S = np.asarray(raw).shape[0]
    return api.ici_kendalltau_pcoa(np.zeros((4, S)), colnames=[f"s{i}" for i in range(S)], engine=RawEngine(raw), **kw)


def _random_raw(S, seed, nan=0):
    rng = np.random.default_rng(seed)
    raw = rng.uniform(-1.0, 1.0, (S, S))
    raw = np.triu(raw, 1) + np.triu(raw, 1).T
    np.fill_diagonal(raw, 1.0)
    for _ in range(nan):
        i, j = rng.choice(S, 2, replace=False)
        raw[i, j] = raw[j, i] = np.nan
    return raw


def _line_raw(x):
    x = np.asarray(x, dtype=np.float64)
    return 1.0 - np.abs(x[:, None] - x[None, :])


def test_abi_names_and_sources():
    header = open(os.path.join(ROOT, "include", "icikt.h")).read()
    for nm in ("icikt_pcoa_f64", "icikt_pcoa_in", "icikt_pcoa_csc"):
        assert nm in _lib.EXPORTS and re.search(r"\bint " + nm + r"\(", header), nm
    for f in ("icikt_pcoa.hip", "icikt_capi_pcoa.cpp"):
        assert os.path.join(ROOT, "icikendalltau_amd", "csrc", f) in _lib.SOURCES
    assert os.path.join(ROOT, "icikendalltau_amd", "csrc", "icikt_ritz.h") in _lib.HEADERS
    assert all(os.path.exists(p) for p in _lib.SOURCES + _lib.HEADERS)
    assert "#define ICIKT_PCOA_MAX_K 64" in header and _lib.PCOA_MAX_K == 64
    assert "#define ICIKT_PCOA_MAX_BASIS 512" in header and _lib.PCOA_MAX_BASIS == 512
    import icikendalltau_amd
    assert icikendalltau_amd.ici_kendalltau_pcoa is api.ici_kendalltau_pcoa


def test_refusals_by_name():
    raw = _random_raw(70, 1)
    for kw, name in (({"k": 0}, "`k`"), ({"k": 70}, "`k`"), ({"k": 65}, "`k`"), ({"k": True}, "`k`"), ({"k": 2.0}, "`k`"),
                     ({"tol": 0}, "`tol`"), ({"tol": -1e-8}, "`tol`"), ({"tol": float("nan")}, "`tol`"),
                     ({"k": 5, "max_basis": 4}, "`max_basis`"), ({"k": 5, "max_basis": 0}, "`max_basis`")):
        eng = RawEngine(raw)
        with pytest.raises(ValueError, match=name):
            api.ici_kendalltau_pcoa(np.zeros((4, 70)), colnames=[f"s{i}" for i in range(70)], engine=eng, **kw)
        assert eng.calls == []                                      # refused before the engine is asked
    with pytest.raises(ValueError, match="at least 2 samples"):
        api.ici_kendalltau_pcoa(np.zeros((4, 1)), colnames=["s0"], engine=RawEngine(np.ones((1, 1))))
    got = _front(raw, k=64, max_basis=64)                           # the largest k there is, and max_basis == k
    assert got["eigenvalues"].shape == (64,) and got["vectors"].shape == (70, 64)
    assert _front(_random_raw(2, 2), k=1)["eigenvalues"].shape == (1,)


def test_the_checker_on_five_points_of_a_line_worked_by_hand():
    """x = 0, 1/8, 1/4, 1/2, 1: raw = 1 - |x_i - x_j| and every (x_i - x_j)^2 are dyadic, so q is exact and so are the
    integers: q_ij = (x_i - x_j)^2 2^50.  By hand: the squared differences in 64ths are
    row 0: 1, 4, 16, 64; row 1: 1, 9, 49; row 2: 4, 36; row 3: 16 -- Q = 200/64 2^50; the row sums R = (85, 60, 45, 45,
    165)/64 2^50; x-bar = 3/8, and G_ij = (x_i - x-bar)(x_j - x-bar) exactly, lambda_1 = sum (x_i - x-bar)^2 = (9 + 4 + 1 + 1 + 25)/64 = 5/8 = Q / (5 2^50), every
    other eigenvalue 0.  The checker's G differs from the exact one by the roundings of the centring alone: the two
    means (<= 2^-54 each: m <= 1), their sum (<= 2^-53), the difference (<= 2^-53), the grand mean (<= 2^-54) and the
    last sum (<= 2^-52), halved: 5.5 2^-54 < 2^-51."""
    x = [Fraction(0), Fraction(1, 8), Fraction(1, 4), Fraction(1, 2), Fraction(1)]
    raw = _line_raw([float(v) for v in x])
    n_val, n_na, Q, R, G = pc.brute_gower(raw)
    unit = 2 ** 50 // 64
    assert (n_val, n_na) == (10, 0) and Q == 200 * unit and R == [85 * unit, 60 * unit, 45 * unit, 45 * unit, 165 * unit]
    assert sum(R) == 2 * Q
    mean = sum(x) / 5
    assert mean == Fraction(3, 8)
    exact = [[(a - mean) * (b - mean) for b in x] for a in x]
    worst = max(abs(Fraction(float(G[i, j])) - exact[i][j]) for i in range(5) for j in range(5))
    print("largest |G - exact|", float(worst), "in units of 2^-54:", float(worst * 2 ** 54))
    assert worst <= Fraction(1, 2 ** 51)
    assert np.array_equal(G, G.T)
    lam1 = sum((a - mean) ** 2 for a in x)
    assert lam1 == Fraction(5, 8) and pc.total_inertia(Q, 5) == float(lam1)      # trace(G) = Q / (S 2^50)
    top, w = pc.largest(G, 3)
    assert abs(top[0] - float(lam1)) <= 1e-15 and np.all(np.abs(w[:-1]) <= 1e-15)
    got = _front(raw, k=3, return_gower=True)
    assert np.array_equal(bits(got["gower"]), bits(G)) and got["sums"]["q_total"] == Q and list(got["sums"]["row_q"]) == R
    assert got["total_inertia"] == float(lam1) and got["n_positive"] >= 1
    want = np.array([float(a - mean) for a in x])
    assert want[4] > 0 and abs(want[4]) == np.abs(want).max()        # the sign rule makes the largest component positive
    assert np.abs(got["coordinates"][:, 0] - want).max() <= 1e-15
    assert abs(got["proportion"][0] - 1.0) <= 1e-15


@pytest.mark.parametrize("S,k", [(2, 1), (3, 2), (23, 5), (70, 10)])
def test_the_front_end_restates_the_rule(S, k):
    raw = _random_raw(S, 10 + S)
    n_val, n_na, Q, R, G = pc.brute_gower(raw)
    got = _front(raw, k=k, return_gower=True)
    assert list(got) == KEYS[:15] + ["gower"] + KEYS[15:]
    assert list(_front(raw, k=k)) == KEYS
    assert (got["n_valid"], got["n_na"]) == (n_val, 0) and got["sums"]["q_total"] == Q and isinstance(got["sums"]["q_total"], int)
    assert got["sums"]["row_q"].dtype == object and list(got["sums"]["row_q"]) == R
    assert np.array_equal(bits(got["gower"]), bits(G)) and np.array_equal(G, G.T)
    top, w = pc.largest(G, k)
    assert np.array_equal(bits(got["eigenvalues"]), bits(top))      # the same G, the same eigh
    assert got["min_ritz"] == w[0] and got["converged"] is True and got["n_basis"] == S and got["n_apply"] == 0
    assert pc.sign_rule_holds(got["vectors"])
    assert np.abs(got["vectors"].T @ got["vectors"] - np.eye(k)).max() <= 1e-12
    assert got["total_inertia"] == pc.total_inertia(Q, S) == float(Fraction(Q, S * 2 ** 50))
    assert abs(np.trace(G) - got["total_inertia"]) <= S * 2.0 ** -48
    assert got["n_positive"] == int((top > 0).sum())
    assert np.array_equal(bits(got["coordinates"]), bits(pc.coordinates(got["vectors"], got["eigenvalues"])))
    assert np.array_equal(bits(got["proportion"]), bits(top / got["total_inertia"]))
    assert got["frobenius"] == float(np.linalg.norm(G)) and got["max_taumax"] == 0.5
    assert list(got["sample_id"]) == [f"s{i}" for i in range(S)]


def test_the_sign_rule_takes_the_first_of_equal_magnitudes():
    V = np.array([[-0.5, 0.5, 0.0], [0.5, -0.5, -1.0], [0.25, 0.5, 1.0]])
    out = api._pcoa_sign(V.copy())
    assert np.array_equal(out, np.array([[0.5, 0.5, 0.0], [-0.5, -0.5, 1.0], [-0.25, 0.5, -1.0]]))
    assert pc.sign_rule_holds(out) and not pc.sign_rule_holds(V)
    # two samples: G = [[a, -a], [-a, a]] and the top vector is (1, -1) / sqrt 2, equal magnitudes: index 0 is positive
    got = _front(_line_raw([0.0, 0.5]), k=1)
    assert got["vectors"][0, 0] > 0 > got["vectors"][1, 0] and abs(got["eigenvalues"][0] - 0.125) <= 1e-16


def test_an_na_pair_makes_every_double_na_and_keeps_the_integers():
    S, k = 23, 4
    raw = _random_raw(S, 3, nan=5)
    n_val, n_na, Q, R, G = pc.brute_gower(raw)
    assert n_na == 5 and G is None
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = _front(raw, k=k, return_gower=True)
    assert sum("PCoA needs every pair" in str(x.message) for x in w) == 1 and len(w) == 1
    assert (got["n_valid"], got["n_na"]) == (n_val, 5) and got["sums"]["q_total"] == Q and list(got["sums"]["row_q"]) == R
    for key in FLOATS + ("gower",):
        assert np.all(bits(got[key]) == bits(na_real())[0]), key
    assert got["coordinates"].shape == (S, k) and got["gower"].shape == (S, S)
    assert got["n_positive"] == 0 and got["converged"] is False and got["n_basis"] == 0


def test_a_call_that_has_not_converged_warns_once():
    class Unconverged(RawEngine):
        def pcoa(self, *a, **kw):
            out = list(super().pcoa(*a, **kw))
            out[10] = False
            return tuple(out)

    raw = _random_raw(23, 4)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = api.ici_kendalltau_pcoa(np.zeros((4, 23)), k=3, colnames=[f"s{i}" for i in range(23)], engine=Unconverged(raw))
    assert len(w) == 1 and "has not converged" in str(w[0].message) and got["converged"] is False
    assert np.all(np.isfinite(got["eigenvalues"]))
