"""The call schedules of tests/call_schedule.py, checked without a device: every condition that makes the schedule test
(tests/test_gpu_call_order.py) decisive holds for every committed schedule, the schedules are functions of their seed,
and the two data sets of one shape share no pair's tau."""
import numpy as np
import pytest

from tests import call_schedule as cs
from tests.oracle_engine import OracleEngine

SCHEDULES = cs.all_schedules()


@pytest.mark.parametrize("name", [n for n in SCHEDULES if n != "hand"])
def test_seeded_schedule_meets_every_condition(name):
    calls = SCHEDULES[name]
    assert cs.violations(calls) == []
    assert len(calls) == 17 * 16 + 1 + 2 * 27


def test_violations_sees_what_is_missing():
    """the checker itself: a schedule with one call taken out or repeated is no longer clean"""
    calls = SCHEDULES["seed1"]
    first_fail = next(i for i, c in enumerate(calls) if c.fail == "c")
    assert any("kind (c)" in v for v in cs.violations(calls[:first_fail] + calls[first_fail + 1:]))
    i = next(i for i, c in enumerate(calls) if c.fail is None and c.entry == "mst")
    assert any("its own answer" in v for v in cs.violations(calls[:i + 1] + calls[i:]))
    assert any("never directly follows" in v for v in cs.violations(calls[:100]))
    no_small = [c for c in calls if c.data != cs.SMALL]
    assert any("before and after the smallest" in v for v in cs.violations(no_small))
    assert cs.violations(cs.hand_written()) != []           # (the hand-written walk promises less: its own list)


def test_hand_written_schedule():
    calls = SCHEDULES["hand"]
    assert cs.hand_written_violations(calls) == []
    assert [cs.n_samp(c.data) for c in calls[::8]] == [300, 3, 130, 130, 300]
    edges = [i for i, c in enumerate(calls) if c.entry == "edges"]
    assert edges[1] == 8 + 1 and cs.n_samp(calls[edges[1]].data) < cs.n_samp(calls[edges[0]].data)


def test_schedules_are_functions_of_their_seed():
    for s in cs.SEEDS:
        assert cs.schedule(s) == SCHEDULES[f"seed{s}"]
    assert len({tuple(SCHEDULES[f"seed{s}"]) for s in cs.SEEDS}) == len(cs.SEEDS) >= 4
    assert cs.hand_written() == SCHEDULES["hand"]


def test_inputs():
    assert {(S, n) for S, n, _kind, _form in cs.DATA.values()} == set(cs.SHAPES)
    for key, (S, n, kind, form) in cs.DATA.items():
        X = cs.dense(key)
        assert X.shape == (n, S) and X.flags.f_contiguous and np.array_equal(X, cs.dense(key), equal_nan=True)
        if kind == "continuous" and S > 8:
            assert np.all(X[:, 5] == 1.0) and np.all(np.isnan(X[:, S - 2]))
            assert 0.05 < np.isnan(np.delete(X, S - 2, axis=1)).mean() < 0.11
        if kind == "tied":
            assert np.unique(X[~np.isnan(X)]).size == 4
        for f in ("f64", "f32", "csc"):
            if f == "f32" and form != "f32":
                continue                                     # (only the float32 data sets hold float32 values)
            M = cs.matrix_in(key, f)
            back = M.toarray() if f == "csc" else np.asarray(M, dtype=np.float64)
            assert np.array_equal(back, X, equal_nan=True)
    dup = cs.matrix_in(cs.DUP, "csc")
    p = dup.indptr[120]
    assert dup.shape == (40, 130) and dup.indices[p] == dup.indices[p + 1] and dup.indptr[121] - p >= 2
    good = cs.matrix_in("a130", "csc")
    assert int(np.sum(dup.indices != good.indices)) == 1
    for S in (3, 65, 130, 300):
        cls, n_class, perms = cs.labellings(S)
        assert n_class == 5 and perms.shape == (cs.N_PERM, S) and cls.min() >= 0 and cls.max() < 5
        if S > 3:
            sizes = np.bincount(cls, minlength=5)
            assert len(set(sizes)) == 5 and sizes[3] == 1    # five unequal classes
        c3, n3 = cs.classes3(S)
        assert n3 == 4 and np.sum(c3 == 3) == 1


@pytest.mark.parametrize("a", ["a130", "a65"])
def test_twin_data_sets_share_no_tau(a):
    """every pair's raw tau differs between the two data sets of a shape (a NaN on one side only differs too): what
    an entry leaves behind for data set 1 is never the answer for data set 2"""
    b = cs.TWIN[a]
    S = cs.n_samp(a)
    iu, ju = np.triu_indices(S, k=1)
    eng = OracleEngine()
    ta = eng.pairs(cs.dense(a), iu, ju, "global", "two.sided", False)[0][:, 0]
    tb = eng.pairs(cs.dense(b), iu, ju, "global", "two.sided", False)[0][:, 0]
    same = (ta == tb) | (np.isnan(ta) & np.isnan(tb))
    print("pairs", len(iu), "NaN in a", int(np.isnan(ta).sum()), "NaN in b", int(np.isnan(tb).sum()), "equal", int(same.sum()))
    assert not same.any()
    assert np.isnan(ta).sum() >= 2 * (S - 1) - 1 and not np.isnan(tb).any()
