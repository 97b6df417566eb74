"""tests/golden/reference_ici_kt.npz -- what the compiled reference answered on the designed matrices of
tests/reference_cases.py -- checked on the CPU: that it is current (regenerated in memory where the compiled reference
is available), that its inputs are the designed ones, that every wrap matrix REACHED its regime (the reference's count
differs from the exact count), and that the CPU oracle reproduces it -- which pins the oracle to the compiled
reference on a machine that has neither the reference's tree nor oracle/_ref.  Only the first test may skip."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import reference as R
from tests import epilogue_checker as E
from tests import reference_cases as C

NA_BITS = np.uint64(0x7FF00000000007A2)
F = {k: i for i, k in enumerate(C.COUNT_FIELDS)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fx():
    return C.load_fixture()


def _pairs(fx, name):
    """[(pair index, x, y)] of one fixture block."""
    if name == "deg":
        return [(k, x, y) for k, (_n, x, y) in enumerate(C.fixture_degenerates(fx))]
    X = C.fixture_matrix(fx, name)
    return [(k, X[:, i], X[:, j]) for k, (i, j) in enumerate(zip(*C.pairs_of(X.shape[1])))]


@pytest.mark.skipif(not R.available(), reason="no compiled reference and no reference tree to build it from")
def test_the_committed_fixture_is_current(fx):
    spec = importlib.util.spec_from_file_location("make_reference_golden",
                                                  os.path.join(os.path.dirname(C.FIXTURE), "make_reference_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = gen.generate()
    assert sorted(fresh) == sorted(fx)
    for k, a in fresh.items():
        assert a.dtype == fx[k].dtype and a.shape == fx[k].shape, k
        same = np.array_equal(bits(a), bits(fx[k])) if a.dtype == np.float64 else np.array_equal(a, fx[k])
        assert same, f"{k}: regenerate tests/golden/reference_ici_kt.npz"


def test_the_inputs_are_the_designed_ones(fx):
    assert os.path.getsize(C.FIXTURE) < 200 * 1024
    for m in C.matrices():
        X = C.fixture_matrix(fx, m.name)
        assert np.array_equal(bits(X), bits(m.X)) and (f"X_{m.name}" in fx) == m.stored
    deg = C.fixture_degenerates(fx)
    assert [n for n, _x, _y in deg] == [n for n, _x, _y in C.degenerates()]
    for (_n, x, y), (_m, x2, y2) in zip(deg, C.degenerates()):
        assert np.array_equal(bits(x), bits(x2)) and np.array_equal(bits(y), bits(y2))
    # the behaviours the shapes are there for
    step = C.matrix("step").X
    both = np.isnan(step[:, 2]) & np.isnan(step[:, 3])
    assert step.shape[0] == 65 and both.sum() >= 10 and (np.isnan(step[:, 4]) & np.isnan(step[:, 5])).sum() == 10
    assert np.signbit(step[:, 1][step[:, 1] == 0]).any() and not np.signbit(step[:, 1][step[:, 1] == 0]).all()
    t1 = C.matrix("t1").X
    assert np.unique(t1[:, 0], return_counts=True)[1].max() == 1100 and np.isnan(t1[:, 1]).sum() == 1100
    assert (np.isnan(t1[:, 1]) & np.isnan(t1[:, 4])).sum() == 900 and np.isnan(t1[:, 4]).sum() == 1100
    t0 = C.matrix("t0").X
    assert np.unique(t0[:, 0], return_counts=True)[1].max() == 1300 and np.isnan(t0[:, 1]).sum() == 1300
    xt = C.matrix("xtie").X
    assert np.unique(xt[:, 0], return_counts=True)[1].max() == 46400 and np.isnan(xt[:, 1]).sum() == 46400
    assert ((xt[:, 0] == 1.3125) & np.isnan(xt[:, 1])).sum() == 46350
    # local != global somewhere in every matrix that has shared missing rows; reasons 1, 2, 3 among the degenerates
    for name in ("step", "t1"):
        assert (fx[f"cnt_{name}"][:, 0, F["n"]] < fx[f"cnt_{name}"][:, 1, F["n"]]).any()
    assert set(fx["reason_deg"].ravel().tolist()) == {0, 1, 2, 3}
    assert all(np.all(fx[f"reason_{n}"] == 0) for n in C.MATRIX_NAMES)
    assert np.array_equal(fx["warn_deg"], np.isin(fx["reason_deg"], (2, 3, 4)).astype(np.int8))     # 1 raises none


def _exact(x, y, persp):
    x2, y2 = C.fill(x, y, persp)
    xs, ys = C.exact_tie_sums(x2), C.exact_tie_sums(y2)
    return {"xtie": xs[0], "x0": xs[1], "x1": xs[2], "ytie": ys[0], "y0": ys[1], "y1": ys[2],
            "ntie": C.exact_joint_ties(x2, y2)}


@pytest.mark.parametrize("name,fields", [("t1", {"x1"}), ("t0", {"x0", "x1"}), ("xtie", {"xtie", "x0", "x1", "ntie"})])
def test_every_wrap_matrix_reached_its_regime(fx, name, fields):
    """The reference's count differs from the exact count (group sizes in Python integers; for the fields the O(n^2)
    enumeration gives -- the three tie counts and dis -- that enumeration too, on the matrices it can afford and on
    one pair of the long one) in the fields the matrix is there for, and `dis`, which no int32 touches below 65 536
    rows, equals the enumeration."""
    cnt = fx[f"cnt_{name}"]
    wrapped = set()
    for k, x, y in _pairs(fx, name):
        for s, persp in enumerate(C.PERSPECTIVES):
            got = {f: int(cnt[k, s, F[f]]) for f in F}
            want = _exact(x, y, persp)
            for f, v in want.items():
                if got[f] != v:
                    assert C.in_int32_regime(x, y, persp), (k, persp, f)
                    wrapped.add(f.replace("y", "x"))                  # (a column counts whichever side it stands on)
            if name != "xtie" or (k, persp) == (0, "global"):
                brute = O.bruteforce(x, y, persp)
                assert brute["dis"] == got["dis"] and (brute["xtie"], brute["ytie"], brute["ntie"]) == \
                    (want["xtie"], want["ytie"], want["ntie"]), (k, persp)
                assert brute["con"] + brute["dis"] + brute["xtie"] + brute["ytie"] - brute["ntie"] == got["tot"]
    assert wrapped >= fields, (wrapped, fields)
    if name == "xtie":
        assert (cnt[:, :, F["xtie"]] < 0).any()                       # xtie goes negative


def test_the_small_matrix_is_outside_every_regime(fx):
    for k, x, y in _pairs(fx, "step"):
        for s, persp in enumerate(C.PERSPECTIVES):
            want = _exact(x, y, persp)
            assert all(int(fx["cnt_step"][k, s, F[f]]) == v for f, v in want.items()) and not C.in_int32_regime(x, y, persp)
            brute = O.bruteforce(x, y, persp)
            assert brute["dis"] == fx["cnt_step"][k, s, F["dis"]]


@pytest.mark.parametrize("name", C.MATRIX_NAMES + ("deg",))
def test_the_oracle_reproduces_the_fixture(fx, name):
    """tau, tau_max and completeness bit for bit, the twelve counts and the reason exact, the NA pattern and payload,
    p at the CPU bar (2 E_CPU scaled units, z from the reference's report)."""
    bound = 2 * E.E_CPU["cases"]
    worst = 0.0
    for k, x, y in _pairs(fx, name):
        for s, persp in enumerate(C.PERSPECTIVES):
            for a, alt in enumerate(C.ALTERNATIVES):
                for c, cont in enumerate(C.CONTINUITY):
                    want = fx[f"out_{name}"][k, s, a, c]
                    out, cnt, reason = O.ici_kt(x, y, persp, alt, cont)
                    where = (name, k, persp, alt, cont)
                    assert reason == fx[f"reason_{name}"][k, s], where
                    assert np.array_equal(bits(out)[[0, 2, 3]], bits(want)[[0, 2, 3]]), where
                    assert np.isnan(out[1]) == np.isnan(want[1]), where
                    if reason:
                        assert np.all(bits(out) == NA_BITS) and np.all(bits(want) == NA_BITS), where
                        continue
                    assert [cnt[f] for f in C.COUNT_FIELDS] == fx[f"cnt_{name}"][k, s].tolist(), where
                    z = float(fx[f"z_{name}"][k, s, c])
                    if np.isnan(want[1]):
                        continue
                    if want[1] >= E.TINY:
                        e = E.scaled_error(out[1], float(want[1]), z)
                        worst = max(worst, e)
                        assert e <= bound, (where, out[1], want[1], e)
                    else:
                        assert abs(out[1] - want[1]) <= bound * (1 + z * z) * E.UNIT * want[1] + 4 * 2.0 ** -1074, where
    print(f"\n{name}: worst scaled p error of the oracle against the fixture {worst:.3f} (bar {bound})")
