"""The device epilogue (k2_epilogue, icikt_epilogue.hip) against the exact reference of tests/epilogue_checker.py.

Every other comparison of the pair engine's p-value is absolute at 1e-10, and most p-values of real data are far below
that: the third branch of the device's pnorm (|z| > 5.657), its coefficient tables and the cut-off at 37.5193 pass those
whatever they hold.  Here the same case set as tests/test_epilogue_reference.py runs through Context.pairs and p is held
on the scaled measure |got - p| / p / ((1 + z^2) 2^-52) to 4 E_CPU, E_CPU the CPU oracle's own measured worst value.

Why 4: the device restatement differs from the oracle's in its two exp calls (arguments exact by construction of xsq;
<= 1 ulp on the device against <= 0.5-1 ulp on the host), in possible FMA contraction in the polynomial loops and the z
arithmetic, and in carrying tau, the variance and z in double where the oracle carries them in long double; sqrt and
divide are correctly rounded on both.  Each is a few 2^-53 in z or in p, amplified by at most 1 + z^2, which is the
measure's own scaling."""
import numpy as np
import pytest

from icikendalltau_amd import _lib
from tests import epilogue_checker as E

pytestmark = pytest.mark.gpu

BOUND = 4 * E.E_CPU["cases"]


def _oracle():
    from oracle import oracle as O
    return O


@pytest.fixture(scope="module")
def oracle_counts():
    """{(case name, perspective, int32_compat): (counts, reasons)} of the CPU oracle (neither depends on the
    alternative or on continuity)."""
    O = _oracle()
    out = {}
    for case in E.cases():
        for persp in case.perspectives:
            for compat in (True, False):
                _o, cnt, rsn = O.ici_pairs(case.X, case.pi, case.pj, persp, int32_compat=compat)
                out[case.name, persp, compat] = (cnt, rsn)
    return out


@pytest.mark.parametrize("flags", [0, _lib.FLAG_EXACT_INT64])
@pytest.mark.parametrize("continuity", [False, True])
@pytest.mark.parametrize("alternative", E.ALTERNATIVES)
def test_epilogue_against_exact(hip_ctx, oracle_counts, alternative, continuity, flags):
    worst = {}
    for case in E.cases():
        for persp in case.perspectives:
            out, cnt, rsn = hip_ctx.pairs(case.X, case.pi, case.pj, persp, alternative, continuity, flags)
            rcnt, rrsn = oracle_counts[case.name, persp, not flags]
            assert not rrsn.any() and np.array_equal(rsn, rrsn), (case.name, persp)
            assert np.array_equal(cnt, rcnt[:, :cnt.shape[1]]), f"{case.name}/{persp}: integer counts differ"
            assert out.shape == (len(case.d), 4) and not np.isnan(out).any()
            E.merge_worst(worst, E.check_call(out, cnt, alternative, continuity, BOUND, f"{case.name}/{persp}"))
    print(f"\ndevice {alternative} continuity={continuity} flags={flags}: p "
          + ", ".join(f"{b} {worst['p'][b]:.3f}" for b in E.BRANCHES[:3])
          + f"; tau {worst['tau']:.2f} ulp, tau_max {worst['tau_max']:.2f} ulp, completeness {worst['completeness']:.2f} ulp")


def _plain():
    case = E.cases()[0]
    assert case.name == "plain"
    return case


def test_matrix_serves_the_same_p(hip_ctx):
    case = _plain()
    out, _cnt, _rsn = hip_ctx.pairs(case.X, case.pi, case.pj)
    out5, _keep, _rc = hip_ctx.matrix(case.X, None, case.pi, case.pj, want_keep=False)
    assert np.array_equal(out5[2][case.pi, case.pj], out[:, 1]) and np.array_equal(out5[2][case.pj, case.pi], out[:, 1])


def test_pair_serves_the_same_p(hip_ctx):
    case = _plain()
    out, _cnt, _rsn = hip_ctx.pairs(case.X, case.pi, case.pj, "global", "less")
    tail = [k for k in np.argsort(out[:, 1]) if 0.0 < out[k, 1] < 1e-12][:3]     # the three smallest p above 0
    assert len(tail) == 3
    for k in tail:
        o, _c, r = hip_ctx.pair(case.X[:, 0], case.X[:, case.pj[k]], "global", "less")
        assert r == 0 and np.array_equal(o, out[k])


def test_pairs_complete_serves_the_same_p(hip_ctx):
    case = _plain()
    assert not np.isnan(case.X).any()
    for alternative in E.ALTERNATIVES:
        out, _cnt, _rsn = hip_ctx.pairs(case.X, case.pi, case.pj, "global", alternative, True)
        outc, _c, rsn = hip_ctx.pairs_complete(case.X, case.pi, case.pj, alternative, True)
        assert not rsn.any() and np.array_equal(outc[:, 1], out[:, 1])
