"""The CPU oracle's pnorm and epilogue against an exact reference (mpmath at 60 digits, tests/epilogue_checker.py).

The oracle's pnorm is the same transcription of Cody's published table as the device's: an error both copies share
passes every device-against-oracle comparison, and every such comparison is absolute at 1e-10 while most p-values of
real data are far below that.  Here the p-value is held RELATIVELY, in both tails, on z from 0 to beyond the cut-off
at 37.5193, and the case set is held to conditions (asserted from the exact reference alone) that keep it from passing
by leaving a branch out.  The bound is twice the oracle's own measured worst value (epilogue_checker.E_CPU)."""
import itertools
import math

import numpy as np
import pytest

from tests import epilogue_checker as E


def _oracle():
    from oracle import oracle as O
    return O


@pytest.fixture(scope="module")
def ref_counts():
    """{(case name, perspective): int64 [P, 11]} without the oracle: dis = d on the untied matrices (what
    perm_with_inversions promises; test_perm_with_inversions holds it to that), plain numpy on the others."""
    out = {}
    for case in E.cases():
        n = case.X.shape[0]
        for persp in case.perspectives:
            if case.name in ("tied", "local"):
                c = [E.pair_counts(case.X[:, 0], case.X[:, j], persp) for j in case.pj]
            else:
                c = [(n, 0, d, 0, 0, 0, 0, 0, 0, 0, n * (n - 1) // 2) for d in case.d]
            out[case.name, persp] = np.array(c, dtype=np.int64)
    return out


def test_perm_with_inversions():
    for n in (1, 2, 3, 5, 8):
        tot = n * (n - 1) // 2
        for d in range(tot + 1):
            p = E.perm_with_inversions(n, d)
            assert sorted(p.tolist()) == list(range(n))
            assert sum(1 for i, j in itertools.combinations(range(n), 2) if p[i] > p[j]) == d
    n, tot = 1000, 499500
    for d in (0, 1, 998, 999, 1000, 123456, tot // 2, tot - 1, tot):
        p = E.perm_with_inversions(n, d)
        assert np.array_equal(np.sort(p), np.arange(n))
        assert E.pair_counts(np.arange(n), p)[2] == d
    with pytest.raises(ValueError):
        E.perm_with_inversions(4, 7)


def test_exact_epilogue_by_hand():
    """Two pairs worked by hand: 5 untied rows with one inversion (S = 8, var = 50 / 3), and a tied pair."""
    ex = E.exact_epilogue((5, 0, 1, 0, 0, 0, 0, 0, 0, 0, 10), "two.sided", False)
    assert float(ex.tau) == 0.8 and float(ex.tau_max) == 1.0 and float(ex.completeness) == 1.0
    assert abs(float(ex.z) - 8 / math.sqrt(50 / 3)) < 1e-15
    assert abs(float(ex.p) - math.erfc(8 / math.sqrt(50 / 3) / math.sqrt(2))) < 1e-16
    ex = E.exact_epilogue((5, 0, 1, 0, 0, 0, 0, 0, 0, 0, 10), "greater", True)
    assert abs(float(ex.z) - 7 / math.sqrt(50 / 3)) < 1e-15 and float(ex.s_adj) == 7.0
    # six rows, the last missing in both columns: fills of 0.9 tie rows 4 and 5 in y; the discordant pairs are
    # (0,2) (0,4) (1,4) (2,4) (3,4), so S = 15 - 1 - 2 + 0 - 10 = 2 globally and 10 - 1 - 1 - 10 = -2 locally
    x, y = np.array([1.0, 1, 2, 3, 4, np.nan]), np.array([2.0, 1, 1, 3, np.nan, np.nan])
    c = E.pair_counts(x, y)
    assert c == (6, 2, 5, 0, 1, 2, 0, 18, 0, 36, 15)
    assert E.pair_counts(x, y, "local") == (5, 1, 5, 0, 1, 1, 0, 18, 0, 18, 10)
    ex = E.exact_epilogue(c, "less", False)
    assert abs(float(ex.tau) - 2 / math.sqrt(14 * 13)) < 1e-16
    var = (30 * 17 - 54) / 18 + 4 / 30
    assert abs(float(ex.z) - 2 / math.sqrt(var)) < 1e-15
    assert abs(float(ex.completeness) - 4 / 6) < 1e-16


def _grid():
    z = list(np.linspace(-37.5, 37.5, 3001))
    for e in E.EDGES + (2.0 ** -53,):
        for s in (e, -e):
            z += [np.nextafter(s, -np.inf), s, np.nextafter(s, np.inf)]
    z += [0.0, -0.0, 1e-17, -1e-17, 37.52, -37.52, 40.0, -40.0, np.inf, -np.inf]
    return [float(v) for v in z]


@pytest.mark.parametrize("lower_tail", [True, False])
def test_oracle_pnorm_against_mpmath(lower_tail):
    O = _oracle()
    bound = 2 * E.E_CPU["grid"]
    worst = dict.fromkeys(E.BRANCHES, 0.0)
    bad = []
    checked = 0
    for z in _grid():
        got = O.pnorm(z, lower_tail)
        want = E.exact_pnorm(z, lower_tail)
        if abs(z) >= E.CUTOFF:                         # beyond the cut-off, +-inf: exactly 0.0 or 1.0
            assert want == 0 or want == 1
            if got != float(want):
                bad.append((z, got, float(want)))
        elif want >= E.TINY:
            e = E.scaled_error(got, want, z)
            worst[E.branch_of(z)] = max(worst[E.branch_of(z)], e)
            if not e <= bound:
                bad.append((z, got, float(want), e))
        else:
            assert abs(got - want) <= bound * (1 + z * z) * E.UNIT * want + 4 * 2.0 ** -1074, (z, got)
        checked += 1
    print(f"\noracle pnorm(lower_tail={lower_tail}) worst scaled error per branch: "
          + ", ".join(f"{b} {worst[b]:.3f}" for b in E.BRANCHES[:3]))
    assert checked == len(_grid()) and not bad, bad[:5]
    assert O.pnorm(0.0, lower_tail) == 0.5 and O.pnorm(-0.0, lower_tail) == 0.5
    assert math.isnan(O.pnorm(float("nan"), lower_tail))


def test_oracle_counts_equal_the_numpy_counts(ref_counts):
    O = _oracle()
    for case in E.cases():
        for persp in case.perspectives:
            for compat in (True, False):
                _out, cnt, rsn = O.ici_pairs(case.X, case.pi, case.pj, persp, int32_compat=compat)
                assert not rsn.any(), (case.name, persp)
                assert np.array_equal(cnt[:, :11], ref_counts[case.name, persp]), (case.name, persp, compat)


def test_case_set_reaches_every_branch(ref_counts):
    """What keeps the comparison below from passing by leaving cases out; everything here comes from the exact
    reference and the counts alone."""
    for name, c in ref_counts.items():
        # reason 0: at least 3 rows here (2 would do), neither column constant, ties below the total
        assert (c[:, 0] >= 3).all() and (c[:, 4] < c[:, 10]).all() and (c[:, 5] < c[:, 10]).all(), name
    for continuity in (False, True):
        z = np.array([float(E.exact_epilogue(row, "less", continuity).z) for c in ref_counts.values() for row in c])
        s = np.array([row[10] - row[4] - row[5] + row[3] - 2 * row[2] for c in ref_counts.values() for row in c])
        for edge in E.EDGES:
            assert np.abs(np.abs(z) - edge).min() > 1e-9, (continuity, edge)
        for sign in (1, -1):
            zs = sign * z[sign * z > 0]
            n_in = {b: sum(1 for v in zs if E.branch_of(v) == b) for b in E.BRANCHES}
            assert min(n_in["small"], n_in["middle"], n_in["tail"]) >= 20 and n_in["cut"] >= 5, (continuity, sign, n_in)
            for edge in E.EDGES:
                assert ((zs > edge) & (zs < edge + 2e-3)).any(), (continuity, sign, edge, "above")
                assert ((zs < edge) & (zs > edge - 2e-3)).any(), (continuity, sign, edge, "below")
        assert (s == 0).any() and (s == 1).any() and (s == -1).any()
    for row in (r for c in ref_counts.values() for r in c):
        if abs(row[10] - row[4] - row[5] + row[3] - 2 * row[2]) <= 1:
            ex = E._exact_core(tuple(int(v) for v in row), True)
            assert ex[4] == 0 and ex[5] == 0                                  # s_adj = 0, z = 0
            assert [float(E.exact_epilogue(row, a, True).p) for a in E.ALTERNATIVES] == [1.0, 0.5, 0.5]


_WORST = {}


@pytest.mark.parametrize("int32_compat", [True, False])
@pytest.mark.parametrize("continuity", [False, True])
@pytest.mark.parametrize("alternative", E.ALTERNATIVES)
def test_oracle_epilogue_against_exact(ref_counts, alternative, continuity, int32_compat):
    O = _oracle()
    bound = 2 * E.E_CPU["cases"]
    worst = {}
    pairs = 0
    for case in E.cases():
        for persp in case.perspectives:
            out, cnt, rsn = O.ici_pairs(case.X, case.pi, case.pj, persp, alternative, continuity, int32_compat)
            assert not rsn.any() and not np.isnan(out).any()
            assert np.array_equal(cnt[:, :11], ref_counts[case.name, persp])
            E.merge_worst(worst, E.check_call(out, ref_counts[case.name, persp], alternative, continuity, bound,
                                              f"{case.name}/{persp}"))
            pairs += out.shape[0]
    assert pairs == sum(c.shape[0] for c in ref_counts.values())             # no p-value is left unchecked
    E.merge_worst(_WORST, worst)
    print(f"\noracle {alternative} continuity={continuity} int32_compat={int32_compat}: p "
          + ", ".join(f"{b} {worst['p'][b]:.3f}" for b in E.BRANCHES[:3])
          + f"; tau {worst['tau']:.2f} ulp, tau_max {worst['tau_max']:.2f} ulp, completeness {worst['completeness']:.2f} ulp"
          + f"; so far overall {max(_WORST['p'].values()):.3f}")
