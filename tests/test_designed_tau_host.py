"""tests/designed_tau.py tied to the two references the project already trusts: its closed-form tau against the CPU
oracle BITWISE (both families, both perspectives, with an all-NaN and a constant column), its per-code reason counts
against the oracle's, and its closed-form answers of the five selection entries against the brute-force checkers fed the
closed-form matrices."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import api
from oracle import oracle as O
from tests import designed_tau as dt
from tests.classmat_checker import brute_class_matrix
from tests.edges_checker import brute_edges
from tests.medians_checker import brute_medians
from tests.oracle_engine import OracleEngine
from tests.quantiles_checker import PROBS, brute_quantiles
from tests.topk_checker import brute_topk

FAMILIES = {"swaps": dt.swaps, "reversals": dt.reversals}
bits = dt.bits


def _design(family, n, S=14, na=True, **kw):
    return FAMILIES[family](S, n, seed=3, n_all_missing=1 if na else 0, n_constant=1 if na else 0, **kw)


@pytest.mark.parametrize("na", [True, False])
@pytest.mark.parametrize("perspective", ["global", "local"])
@pytest.mark.parametrize("n", [40, 41])
@pytest.mark.parametrize("family", ["swaps", "reversals"])
def test_closed_form_is_the_oracle_bitwise(family, n, perspective, na):
    d = _design(family, n, na=na)
    S = d.S
    assert len(np.unique(np.abs(d.num[d.valid]))) >= 5 and np.any(d.num < 0) and np.any(d.sign == -1)
    names = [f"s{i}" for i in range(S)]
    for scale_max in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            full = api.ici_kendalltau(d.X, perspective=perspective, scale_max=scale_max, colnames=names,
                                      engine=OracleEngine())
        raw, cor, taumax = (np.asarray(full[k]) for k in ("raw", "cor", "taumax"))
        off = ~np.eye(S, dtype=bool)
        assert np.array_equal(np.isnan(raw[off]), ~d.valid[off])
        assert np.array_equal(bits(raw[d.valid]), bits(d.raw[d.valid]))
        assert np.array_equal(bits(cor[d.valid]), bits(d.raw[d.valid]))
        assert np.all(taumax[d.valid] == 1.0) and np.all(np.asarray(full["completeness"])[d.valid] == 1.0)
    # the pair list as the library takes it: values and reason codes per pair
    iu, ju = np.triu_indices(S, k=1)
    out, _cnt, rsn = O.ici_pairs(d.X, iu.astype(np.int32), ju.astype(np.int32), perspective=perspective)
    assert np.array_equal(rsn, d.reasons()[iu, ju])
    assert np.array_equal(np.bincount(rsn, minlength=5), d.reason_counts())
    assert d.reason_counts().sum() == S * (S - 1) // 2
    if na:
        assert d.reason_counts().tolist() == [(S - 2) * (S - 3) // 2, S - 1, 0, S - 2, 0]
    ok = rsn == 0
    assert np.array_equal(bits(out[ok, 0]), bits(d.raw[iu, ju][ok])) and np.all(out[ok, 2] == 1.0)
    assert d.max_taumax() == 1.0


def test_discordance_formulas_by_counting():
    """D of both families by the definition: row pairs that the two columns order differently"""
    for family, n in (("swaps", 9), ("reversals", 10)):
        d = FAMILIES[family](12, n, seed=5)
        r, s = np.triu_indices(n, k=1)
        for a in range(d.S):
            for b in range(d.S):
                if a == b:
                    continue
                conc = np.sign(d.X[r, a] - d.X[s, a]) * np.sign(d.X[r, b] - d.X[s, b])
                assert int(conc.sum()) == d.num[a, b], (family, a, b)


def _classes(d, seed=2):
    """three seeded classes, and class 3 = the NA columns alone"""
    cls = np.random.default_rng(seed).integers(0, 3, d.S).astype(np.int32)
    cls[d.kind != dt.VALID] = 3
    return cls, 4


@pytest.fixture(scope="module", params=[("swaps", 40, 14), ("reversals", 41, 14), ("swaps", 8, 37), ("reversals", 7, 37)],
                ids=lambda p: "%s-n%d-S%d" % p)
def design(request):
    """S = 14 as the oracle comparison runs it; S = 37 with 8 and 7 rows has few distinct values: long runs of ties"""
    family, n, S = request.param
    return FAMILIES[family](S, n, seed=3, n_all_missing=1, n_constant=1)


def test_topk_against_the_checker(design):
    d = design
    for k in (1, 3, d.S - 3, d.S + 4):
        idx, nums, raw, n_valid = dt.topk(d, k)
        ridx, rvals, rn = brute_topk([d.raw] * 5, k)
        assert np.array_equal(idx, ridx) and np.array_equal(n_valid, rn)
        assert np.array_equal(bits(raw), bits(rvals[1]))
        assert np.array_equal(bits(dt.na_filled(raw.shape))[idx < 0], bits(raw)[idx < 0])
        assert np.array_equal(bits(d.value(nums))[idx >= 0], bits(raw)[idx >= 0])
    na_cols = np.nonzero(d.kind != dt.VALID)[0]
    assert np.all(n_valid[na_cols] == 0) and np.all(idx[na_cols] == -1)


def test_edges_against_the_checker(design):
    d = design
    vals = np.unique(d.num[d.valid])
    for t in (int(vals[len(vals) // 2]), int(vals[-1]), int(vals[0]), 1, d.m + 1):
        for absolute in (False, True):
            ei, ej, nums, raw, n_edges, degree = dt.edges(d, t, absolute)
            rei, rej, rvals, rn, rdeg = brute_edges([d.raw] * 5, min_raw=t / float(d.m), absolute=absolute)
            assert n_edges == rn and np.array_equal(ei, rei) and np.array_equal(ej, rej)
            assert np.array_equal(degree, rdeg) and np.array_equal(bits(raw), bits(rvals[1]))
    assert n_edges == 0


def test_medians_against_the_checkers(design):
    d = design
    cls, n_class = _classes(d)
    for c, nc in ((None, 1), (cls, n_class)):
        cm = dt.class_matrix(d, c, nc)
        med2, n_valid = brute_class_matrix([d.raw] * 5, c, nc)
        assert np.array_equal(cm["n_valid"], n_valid)
        assert np.array_equal(bits(cm["med"]), bits(med2[1])) and np.array_equal(bits(cm["med"]), bits(med2[0]))
        own = dt.class_medians(d, c)
        med2, n_valid = brute_medians([d.raw] * 5, c)
        assert np.array_equal(own["n_valid"], n_valid) and np.array_equal(bits(own["med"]), bits(med2[1]))
        # the run bookkeeping: lo is at rank k_in of `run` equal numerators, hi the next rank's
        have = cm["n_valid"] > 0
        assert np.all(cm["k_in"][have] < cm["run"][have]) and np.all(cm["hi"] >= cm["lo"])
        inside = have & (cm["n_valid"] % 2 == 0) & (cm["k_in"] + 1 < cm["run"])
        assert np.all(cm["hi"][inside] == cm["lo"][inside])
        edge = have & (cm["n_valid"] % 2 == 0) & (cm["k_in"] + 1 == cm["run"])
        assert np.all(cm["hi"][edge] > cm["lo"][edge])
    assert np.all(cm["n_valid"][:, 3] == 0) and np.all(bits(cm["med"][:, 3]) == dt.NA_REAL_BITS)


def test_quantiles_and_histogram_against_the_checker(design):
    d = design
    cls, _n_class = _classes(d)
    vals = np.unique(d.num[d.valid])
    break_sets = [np.array([-d.m, 0, d.m]), np.array([int(vals[0]), int(vals[-1])]),
                  vals[1:-1] if len(vals) > 3 else vals, np.arange(-d.m - 4, d.m + 6, 3), np.array([1, 2])]
    for c in (None, cls):
        counts = dt.group_counts(d, c)
        q, order2, ord_num, n_valid, n_na = dt.quantiles(d, PROBS, c, counts)
        for bn in break_sets:
            hist, outside = dt.histogram(d, bn, c, counts)
            rq2, rorder2, rnv, rna, rhist, rout = brute_quantiles([d.raw] * 5, c, PROBS, bn / float(d.m))
            assert np.array_equal(hist, rhist) and np.array_equal(outside, rout), bn
            assert np.array_equal(hist.sum(axis=1) + outside.sum(axis=1), n_valid)
        assert np.array_equal(n_valid, rnv) and np.array_equal(n_na, rna)
        assert np.array_equal(bits(order2), bits(rorder2))
        assert np.array_equal(bits(q), bits(rq2[1])) and np.array_equal(bits(q), bits(rq2[0]))
        assert np.array_equal(bits(d.value(ord_num))[:, :, 0][n_valid > 0], bits(order2)[:, :, 0][n_valid > 0])
    assert n_na[1] == 1 and n_valid[1] + n_valid[2] == n_valid[0]      # the NA class's one pair is a within pair
