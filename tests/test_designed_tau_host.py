"""tests/designed_tau.py tied to the two references the project already trusts: its closed-form tau against the CPU
oracle BITWISE (both families, both perspectives, with an all-NaN and a constant column), its per-code reason counts
against the oracle's, and its closed-form answers of the five selection entries against the brute-force checkers fed the
closed-form matrices.  Below those, the references of the seven later entries (anosim, permanova, padjust, mst, cross and
its class table) against their checkers at S = 130, permdisp's table and dict against its checker with what the large
GPU tests presuppose about their inputs, and the mutations that the designs of the GPU tests must keep showing: two
replayed defects of permdisp's sweep and hclust's contracted average update.  At the end the censored family: against
the oracle, by direct counting, against the checkers, and five replayed defects of scaling, carrying and perspective."""
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

from icikendalltau_amd import api
from oracle import oracle as O
from tests import anosim_checker, cross_checker, hclust_checker, mst_checker, padjust_checker, permanova_checker
from tests import designed_tau as dt
from tests.classmat_checker import brute_class_matrix
from tests.cross_class_checker import brute_cross_class
from tests.edges_checker import brute_edges
from tests.medians_checker import brute_medians
from tests.oracle_engine import OracleEngine
from tests.quantiles_checker import PROBS, brute_quantiles
from tests import test_gpu_designed_tau as gpu_base
from tests.test_gpu_designed_tau import _design as _gpu_design      # the S = 130 designs the GPU tests use
from tests.test_gpu_designed_tau_entries import _design as _entries_design, _layout as _entries_layout   # and the later ones
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


# ---- the seven later entries: anosim, permanova, padjust, mst, hclust, cross and its class table -----------------------
# S = 130 on the designs of tests/test_gpu_designed_tau_entries.py, each new reference against the brute-force checker
# fed the closed-form matrix (or, for the p-values and the rectangle, the CPU oracle's).

KEYS130 = ["two-valued", "two-valued-half", "swaps40", "reversals41", "reversals41-wide"]


def _same_item(a, b, name):
    if isinstance(a, np.ndarray) and a.dtype == np.float64:
        assert np.array_equal(bits(a), bits(np.asarray(b, dtype=np.float64))), name
    elif isinstance(a, float):
        assert bits(np.array([a]))[0] == bits(np.array([b]))[0], name
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), name
    else:
        assert a == b, name


def _four_classes(d, seed, na_class):
    cls = np.random.default_rng(seed).integers(0, 3, d.S).astype(np.int32)
    if na_class:
        cls[d.kind != dt.VALID] = 3
    else:
        cls[::9] = 3
    return cls, 4


@pytest.mark.parametrize("na", [True, False])
@pytest.mark.parametrize("key", KEYS130)
def test_anosim_and_permanova_against_the_checkers(key, na):
    d = _gpu_design(key) if na else dt.valid_columns(_gpu_design(key))
    for na_class in (True, False):
        cls, n_class = _four_classes(d, 5, na_class and na)
        perms = anosim_checker.documented_permutations(cls, 7, seed=11)
        got, want = dt.anosim(d, cls, n_class, perms), anosim_checker.brute_anosim(d.raw, cls, n_class, perms)
        for name in got:
            _same_item(got[name], want[name], name)
        assert got["n_pairs"][0] > 0 and (got["n_pairs"][1] > 0) == na and want["exact"][0] is not None
        got, want = dt.permanova(d, cls, n_class, perms), permanova_checker.brute_permanova(d.raw, cls, n_class, perms)
        for name in got:
            _same_item(got[name], want[name], name)
        assert got["q_total"] > 0 and (want["exact"][0][0] is None) == na
        if not na:
            assert all(any(row) for row in got["class_q"])
    if key.startswith("two-valued"):
        table = dt.q_table(d)
        assert table[0] == 2 ** 52 and table[2 * d.m] == 0           # raw = -1 and +1: the ends of q's range


def _oracle_pvalues(d, perspective, alternative):
    iu, ju = np.triu_indices(d.S, k=1)
    out, _cnt, _rsn = O.ici_pairs(d.X, iu.astype(np.int32), ju.astype(np.int32), perspective=perspective,
                                  alternative=alternative, want_counts=False)
    plane = np.full((d.S, d.S), np.nan)
    plane[iu, ju] = out[:, 1]
    return plane


@pytest.mark.parametrize("alternative", ["two.sided", "greater"])
@pytest.mark.parametrize("key", KEYS130)
def test_sorted_pvalues_against_the_checker(key, alternative):
    d = _gpu_design(key)
    one_sided = alternative != "two.sided"
    plane = _oracle_pvalues(d, "global", alternative)
    i, j, k, n_na = dt.triangle(d)
    keys, count, fi, fj, _n_na = dt.pvalue_keys(d, one_sided)
    num = k.astype(np.int64) - d.m
    at = np.searchsorted(keys, num if one_sided else np.abs(num))
    p_of_key = plane[fi, fj]
    assert not np.isnan(p_of_key).any()
    assert np.array_equal(bits(plane[i, j]), bits(p_of_key[at]))      # p is a function of the key alone on the design
    assert count.sum() == len(i) and count.max() >= 100
    p, got_na = dt.sorted_pvalues(d, p_of_key, one_sided)
    want, want_na = padjust_checker.sorted_tests(plane)
    assert got_na == want_na == n_na and np.array_equal(bits(p), bits(want))
    kinds = set()
    for method in padjust_checker.METHODS:
        fast = padjust_checker.outputs_from_sorted(p, n_na, method)
        slow = padjust_checker.outputs_from_sorted(p, n_na, method, fast=False)
        for name in fast:
            _same_item(fast[name], slow[name], name)
        # equal p-values have equal adjusted values: every cut lies between two runs
        n = fast["n_rejected"]
        inner = n[(n > 0) & (n < len(p))]
        assert np.all(p[inner - 1] != p[inner])
        kinds |= set(dt.cuts_in_runs(p, method, padjust_checker.ALPHAS))
        a_in = dt.alpha_inside_a_run(p, method)
        assert (a_in is None) == (method == "bonferroni")
        if a_in is not None:   # a level inside a run's unscanned products: the whole run still falls on one side
            assert 0.0 < a_in <= 1.0 and dt.cuts_in_runs(p, method, (a_in,)) == ["inside"]
            n_in = padjust_checker.outputs_from_sorted(p, n_na, method, (a_in,), fast=False)["n_rejected"][0]
            assert n_in in (0, len(p)) or p[n_in - 1] != p[n_in]
    print(key, alternative, "cuts at the five levels", kinds)
    if key == "reversals41-wide":
        assert "edge" in kinds


@pytest.mark.parametrize("S", [130, 257, 520])
def test_mst_two_valued_against_kruskal(S):
    for n_na in ((0, 3) if S == 130 else (0,)):
        rng = np.random.default_rng(S)
        signs = np.where(rng.random(S - n_na) < 0.4, -1, 1)
        d = dt.swaps(S, 24, seed=S, params=np.zeros(S - n_na, dtype=np.int64), signs=signs, n_all_missing=n_na // 3,
                     n_constant=n_na - n_na // 3)
        assert dt.is_two_valued(d) and set(np.unique(d.num[d.valid]).tolist()) == {-d.m, d.m}
        ti, tj, component, n_comp = dt.mst_two_valued(d)
        rti, rtj, rcomponent, rn = mst_checker.brute_mst(d.raw)
        assert np.array_equal(ti, rti) and np.array_equal(tj, rtj) and np.array_equal(component, rcomponent) and n_comp == rn
        assert n_comp == 1 + n_na and int(np.sum(d.num[ti, tj] < 0)) == 1
        if S == 130:
            assert mst_checker.verify_forest(d.raw, ti, tj, component) == n_comp
    d = _gpu_design("two-valued")
    got, want = dt.mst_two_valued(d), mst_checker.brute_mst(d.raw)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert mst_checker.verify_forest(d.raw, got[0], got[1], got[2]) == 10
    assert not dt.is_two_valued(_gpu_design("swaps40"))
    got, want = dt.mst_two_valued(_gpu_design("swaps40")), mst_checker.brute_mst(_gpu_design("swaps40").raw)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("perspective", ["global", "local"])
@pytest.mark.parametrize("key", KEYS130)
def test_rectangle_against_the_checkers(key, perspective):
    d = _gpu_design(key)
    Sq = 7
    r = dt.rect(d, Sq)
    pi, pj = cross_checker.rect_pairs(Sq, r.Sr)
    out, _cnt, rsn = O.ici_pairs(d.X, pi, pj, perspective=perspective, want_counts=False)
    raw, p, taumax, comp = (np.ascontiguousarray(out[:, f].reshape(Sq, r.Sr)) for f in range(4))
    assert np.array_equal(rsn.reshape(Sq, r.Sr), r.reasons) and np.array_equal(np.isnan(raw), ~r.valid)
    assert np.array_equal(bits(raw[r.valid]), bits(r.raw[r.valid])) and np.all(taumax[r.valid] == 1.0)
    assert np.array_equal(np.bincount(rsn, minlength=5), r.reason_counts())
    rect5 = [raw, raw, p, taumax, comp]
    assert cross_checker.max_taumax(rect5) == r.max_taumax()
    for k in (1, 7, r.Sr):
        idx, nums, topraw, n_valid = dt.cross_topk(d, Sq, k)
        ridx, rvals, rn = cross_checker.brute_cross_topk(rect5, k)
        assert np.array_equal(idx, ridx) and np.array_equal(n_valid, rn) and np.array_equal(bits(topraw), bits(rvals[1]))
    ref_cls = np.random.default_rng(3).integers(0, 3, r.Sr).astype(np.int32)
    ref_cls[ref_cls == 2] = 3                                          # class 2 empty
    ref_cls[d.kind[Sq:] != dt.VALID] = 4                               # a class of NA columns alone
    cm = dt.cross_class_table(d, Sq, ref_cls, 5)
    med2, n_valid = brute_cross_class(rect5, ref_cls, 5)
    assert np.array_equal(cm["n_valid"], n_valid)
    assert np.array_equal(bits(cm["med"]), bits(med2[1])) and np.array_equal(bits(cm["med"]), bits(med2[0]))
    assert np.all(n_valid[:, [2, 4]] == 0) and np.all(bits(cm["med"][:, [2, 4]]) == dt.NA_REAL_BITS)


# ---- permdisp: the reference against the checker, what the GPU tests presuppose, and two defects replayed --------------

@pytest.mark.parametrize("classes", ["interleaved", "na-class"])
@pytest.mark.parametrize("na", [True, False])
@pytest.mark.parametrize("key", KEYS130)
def test_permdisp_against_the_checker(key, na, classes):
    from tests import permdisp_checker
    d = _entries_design(key if na else key + "/valid")
    cls, n_class = _entries_layout(d, key if na else key + "/valid", classes)
    perms = permdisp_checker.documented_permutations(cls, 7, seed=11)
    n_val, n_na, Q, T, A, sizes = dt.permdisp_table(d, cls, n_class)
    want = permdisp_checker.brute_table(d.raw, cls, n_class)
    assert T.dtype == object and T.shape == (d.S, n_class) and all(type(v) is int for v in T.ravel())
    assert (n_val, n_na, Q, T.tolist(), A, sizes) == want
    assert (n_na > 0) == na and Q > 0 and all(type(v) is int for v in [n_val, n_na, Q] + A + sizes)
    lo, hi = dt.permdisp_limbs(d, cls, n_class)
    assert lo.dtype == hi.dtype == np.int64 and np.array_equal(dt.limbs_to_ints(lo, hi), T)
    got, ref = dt.permdisp(d, cls, n_class, perms), permdisp_checker.brute_permdisp(d.raw, cls, n_class, perms)
    assert set(got) == set(ref)
    for name in got:
        if name not in ("exact", "x", "residuals"):
            _same_item(got[name], ref[name], name)
    assert got["exact"] == ref["exact"] and got["x"] == ref["x"] and (na or got["residuals"] == ref["residuals"])
    assert (ref["exact"][0][0] is None) == na
    pv = dt.permanova(d, cls, n_class, perms)
    assert Q == pv["q_total"] and np.array_equal(pv["n_pairs"], [n_val, n_na])
    if na:   # the table is as summed; PERMANOVA's class sums are not
        assert any(A) and not any(pv["class_q"][0]) and T[d.kind == dt.VALID].any() and not T[d.kind != dt.VALID].any()
    else:
        assert A == pv["class_q"][0]


def test_the_inputs_of_the_large_permdisp_tests_are_what_they_presuppose():
    from tests.test_gpu_medians import _five_classes
    d = _entries_design("rev24-5794")
    cls, n_class = _five_classes(d.S)
    lo, hi = dt.permdisp_limbs(d, cls, n_class)
    good = d.kind == dt.VALID
    print("cells of valid samples", lo[good].size, "lo-limb sums from", int(lo[good].min()).bit_length(), "to",
          int(lo.max()).bit_length(), "bits, hi up to", int(hi.max()).bit_length(), "bits")
    assert good.sum() == d.S - 2 and lo[good].min() >= 1 << 32 and not lo[~good].any() and not hi[~good].any()
    assert lo.max() < 1 << 48 and hi.max() < 1 << 36                                  # icikt_permdisp.hip's bounds
    d = _entries_design("halves-2049")
    T = dt.permdisp_table(d, np.zeros(d.S, dtype=np.int32), 1)[3]
    assert T[:1024, 0].tolist() == [1025 << 52] * 1024 and T[1024:, 0].tolist() == [1024 << 52] * 1025


def _lost_carry(d, cls, n_class):
    """a cell's lo limb kept modulo 2^32"""
    lo, hi = dt.permdisp_limbs(d, cls, n_class)
    return lo & 0xFFFFFFFF, hi


def _column_role_one_to_the_right(d, cls, n_class):
    """k_disp_table's column role (the partners t < s of sample s) reading the pair (t, s + 1) in place of (t, s): the
    next key of row t in the kept plane -- behind the row's last pair (s = S - 1) that is the first pair of row t + 1,
    (t + 1, t + 2), and behind the plane nothing (no value).  The row role (t > s) is as it was.  The sweep is
    dt.permdisp_limbs on the planes so read."""
    import copy
    S = d.S
    num, valid = d.num.copy(), d.valid.copy()
    low = np.tril(np.ones((S, S), dtype=bool), -1)
    for plane, src in ((num, d.num), (valid, d.valid)):
        below = np.empty_like(src)
        below[:-1] = src[1:]                                           # [s, t] <- [s + 1, t] == (t, s + 1)
        below[-1] = 0
        below[-1, :S - 2] = src[np.arange(1, S - 1), np.arange(2, S)]  # [S - 1, t] <- (t + 1, t + 2)
        plane[low] = below[low]
    read = copy.copy(d)
    read.num, read.valid = num, valid
    return dt.permdisp_limbs(read, cls, n_class)


def _cells(lo, hi):
    """hi 2^32 + lo in int64: the designs' hi sums stay below 2^31 - 2^16 (1 025 x 2^20 is the largest)"""
    assert hi.max() < (1 << 31) - (1 << 16) and lo.max() < 1 << 48
    return (hi << 32) + lo


def _replay_labels(key):
    from tests.test_gpu_designed_tau_entries import PMV_LDS_CLASSES, _classes_of_two
    from tests.test_gpu_medians import _five_classes
    d = _entries_design(key)
    if d.S == 130:
        return _entries_layout(d, key, "interleaved")
    if key == "halves-2049":
        return (np.arange(d.S) >= 1024).astype(np.int32), 2
    if key == "rev24-4098":
        return _classes_of_two(d.S, PMV_LDS_CLASSES), PMV_LDS_CLASSES
    return _five_classes(d.S)


REPLAY_DESIGNS = KEYS130 + ["rev24-2049", "halves-2049", "rev24-4098", "rev24-5794"]


@pytest.mark.parametrize("key", REPLAY_DESIGNS)
def test_two_replayed_permdisp_defects_show_on_the_designs(key):
    """The guard that the designs of the GPU tests can see (a) a carry lost between a cell's limbs and (b) a column
    role that reads its neighbour's pair.  (a) cannot show where every q is 0 or 2^52 (lo limb 0); (b) cannot show in a
    row of a two-valued design whose neighbour has the same sign and kind.  That is why every size also runs a design
    of prefix reversals, on which both change most rows of the table."""
    d = _entries_design(key)
    cls, n_class = _replay_labels(key)
    lo, hi = dt.permdisp_limbs(d, cls, n_class)
    T, carry, shifted = (_cells(*planes) for planes in ((lo, hi), _lost_carry(d, cls, n_class),
                                                         _column_role_one_to_the_right(d, cls, n_class)))
    rows_carry = np.nonzero((carry != T).any(axis=1))[0]
    rows_shift = np.nonzero((shifted != T).any(axis=1))[0]
    print(key, "rows of the table that change: lost carry", len(rows_carry), "column role", len(rows_shift), "of", d.S)
    if dt.is_two_valued(d):
        assert len(rows_carry) == 0 and not lo.any()
        nxt = np.arange(d.S) + 1
        may = (nxt == d.S) | (d.sign != d.sign[np.minimum(nxt, d.S - 1)]) | (d.kind != d.kind[np.minimum(nxt, d.S - 1)])
        assert len(rows_shift) > 0 and may[rows_shift].all() and not may.all()
    else:
        assert len(rows_carry) > d.S // 2 and len(rows_shift) > d.S // 2
    if key in ("rev24-4098", "rev24-5794"):
        gpu_base._DESIGN.pop(key, None)                               # (a third of a gigabyte; the GPU tests build it again)


# ---- a mutation that must keep failing: average linkage with one product fused into the sum --------------------------

def _round(x):
    return float(x)                     # Fraction -> float rounds once, to nearest even


def _contracted(which):
    """average_update with one product kept exact inside the sum (a fused multiply-add): four roundings, not five"""
    def update(na, wa, nb, wb):
        if which == "first":
            s = _round(Fraction(na) * Fraction(wa) + Fraction(nb * wb))
        else:
            s = _round(Fraction(na * wa) + Fraction(nb) * Fraction(wb))
        return s / (na + nb)
    return update


AVERAGE_DESIGNS = {
    "rev24-520": lambda: dt.reversals(520, 24, seed=3),      # the GPU test's design for average linkage
    "reversals41-wide": lambda: _gpu_design("reversals41-wide"),
    "swaps40": lambda: _gpu_design("swaps40"),
}


@pytest.mark.parametrize("which", ["first", "second"])
@pytest.mark.parametrize("key", list(AVERAGE_DESIGNS))
def test_a_contracted_average_update_shows_on_the_designs(key, which):
    """The guard that the designs of the GPU test can see an hc_update that the compiler contracted: DESIGN.md section
    22 records a build that did.  If a design is changed, it must be changed to one for which this still holds."""
    d = AVERAGE_DESIGNS[key]()
    want = hclust_checker.brute_hclust(d.raw, "average")
    got = hclust_checker.brute_hclust(d.raw, "average", average=_contracted(which))
    n = min(len(want[0]), len(got[0]))
    order = int(np.sum((want[0][:n] != got[0][:n]) | (want[1][:n] != got[1][:n])))
    heights = int(np.sum(bits(want[3][:n]) != bits(got[3][:n])))
    print(key, which, "merges that differ", order, "heights that differ", heights)
    assert order + heights > 0
    if key == "rev24-520" and which == "first":
        assert order > 0                                               # the merge order itself changes
    assert math.isfinite(want[3][0])


# ---- the third family: tied, left-censored columns -------------------------------------------------------------------
# taumax != 1, completeness != 1, cor != raw, den varying per pair under "local": what the two families above cannot show.

from tests import epilogue_checker as E          # noqa: E402

CENSORED_SHAPES = {41: (41, 7, 2, 4), 64: (64, 8, 3, 5)}                 # n: (n, B0, c, t)
CENS130 = ["cens64", "cens64-ties", "cens64-apart"]                     # the S = 130 designs of the GPU files


def _ulp_of_fraction(got, num, den):
    """|got - num / den| in units of the spacing of doubles at num / den, exactly"""
    exact = Fraction(int(num), int(den))
    return abs(Fraction(float(got)) - exact) / Fraction(float(np.spacing(float(exact) or 1.0)))


@pytest.mark.parametrize("na", [True, False])
@pytest.mark.parametrize("variant", ["nan", "ties"])
@pytest.mark.parametrize("perspective", ["global", "local"])
@pytest.mark.parametrize("n", [41, 64])
def test_censored_closed_form_is_the_oracle(n, perspective, variant, na):
    d = dt.censored(14, *CENSORED_SHAPES[n], seed=3, variant=variant, n_lib=4, n_all_missing=1 if na else 0,
                    n_constant=1 if na else 0).under(perspective)
    S = d.S
    assert d.n <= 200 and d.distinct_doubles                              # distinct fractions are distinct doubles
    iu, ju = np.triu_indices(S, k=1)
    out, cnt, rsn = O.ici_pairs(d.X, iu.astype(np.int32), ju.astype(np.int32), perspective=perspective)
    assert np.array_equal(rsn, d.reasons()[iu, ju]) and np.array_equal(np.bincount(rsn, minlength=5), d.reason_counts())
    ok = rsn == 0
    a, b = iu[ok], ju[ok]
    assert np.array_equal(ok, d.valid[iu, ju]) and len(a) >= 66
    counts = d.counts(a, b)
    assert np.array_equal(cnt[ok][:, :11], counts)                        # all eleven counts
    tot, xtie, ntie, dis = counts[:, 10], counts[:, 4], counts[:, 3], counts[:, 2]
    assert np.array_equal(d.plus(a, b), tot - 2 * xtie + ntie) and np.array_equal(d.num[a, b], tot - 2 * xtie + ntie - 2 * dis)
    assert np.array_equal(d.den(a, b), tot - xtie) and np.array_equal(d.n_eff(a, b), counts[:, 0])
    assert np.array_equal(bits(out[ok, 0]), bits(d.raw[a, b])) and np.array_equal(bits(out[ok, 2]), bits(d.taumax(a, b)))
    assert np.array_equal(bits(d.raw[a, b]), bits(d.num[a, b] / d.den(a, b).astype(np.float64)))     # one division
    tm = d.taumax(a, b)
    assert tm.max() == d.max_taumax() == 1.0 and np.sum(tm < 1.0) > 50 and tm.min() > 0.99
    assert np.all(d.taumax(a, b)[(d.cols.st[a] == d.cols.st[b]) & (d.cols.lb[a] == d.cols.lb[b])] == 1.0)
    # completeness: the oracle divides in long double and rounds twice, the closed form is 1.0 - missing / n_eff
    miss, ne = d.missing(a, b), d.n_eff(a, b)
    for got in (out[ok, 3], d.completeness(a, b)):
        assert max(_ulp_of_fraction(g, e - m_, e) for g, m_, e in zip(got, miss, ne)) <= 1
    two = (ne & (ne - 1)) == 0
    assert np.array_equal(bits(out[ok, 3][two]), bits(d.completeness(a, b)[two]))
    assert two.all() == (n == 64 and (perspective == "global" or variant == "ties"))
    assert (miss.max() > 0) == (variant == "nan") and (variant == "ties" or d.completeness(a, b).max() < 1.0 or perspective == "local")
    # the p-value: one per distinct (num, den, n_eff) -- per (|num|, den, n_eff) two-sided --, and the exact epilogue's
    for alternative, one_sided in (("two.sided", False), ("greater", True)):
        pv = O.ici_pairs(d.X, a.astype(np.int32), b.astype(np.int32), perspective=perspective, alternative=alternative,
                         want_counts=False)[0]
        ids, first, inv = np.unique(d.pvalue_id(a, b, one_sided), return_index=True, return_inverse=True)
        assert np.array_equal(bits(pv[:, 1]), bits(pv[first, 1][inv])) and 20 <= len(ids) < len(a)
        worst = E.check_call(pv, counts, alternative, False, 2 * E.E_CPU["cases"])
        assert worst["tau"] <= 0.5 and worst["tau_max"] <= 0.5 and worst["completeness"] <= 1.0    # correctly rounded
    # the matrices as the front end scales them
    names = [f"s{i}" for i in range(S)]
    for scale_max in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            full = api.ici_kendalltau(d.X, perspective=perspective, scale_max=scale_max, colnames=names, engine=OracleEngine())
        want = d.planes(None, scale_max)
        for k, name in ((0, "cor"), (1, "raw"), (3, "taumax")):
            got = np.asarray(full[name])
            assert np.array_equal(bits(got[d.valid]), bits(want[k][d.valid])), (name, scale_max)
            assert np.all(np.isnan(got[~d.valid & ~np.eye(S, dtype=bool)]))


def test_censored_formulas_by_counting():
    """num, plus and all eleven counts of the censored family by the definition, on a 9-row and a 10-row example: every
    row pair compared in both columns after the reference's fill (tests/epilogue_checker.pair_counts, plain numpy)"""
    for shape in ((9, 3, 1, 1), (10, 4, 2, 1)):
        for variant in ("nan", "ties"):
            d0 = dt.censored(12, *shape, seed=5, variant=variant, n_lib=3, n_states=3, distinct=False, twin=False)
            for perspective in ("global", "local"):
                d = d0.under(perspective)
                for a in range(d.S):
                    for b in range(d.S):
                        if a == b:
                            continue
                        x, y = d.X[:, a], d.X[:, b]
                        assert E.pair_counts(x, y, perspective) == tuple(d.counts(a, b).tolist()), (shape, variant, a, b)
                        keep = ~(np.isnan(x) & np.isnan(y)) if perspective == "local" else np.ones(len(x), dtype=bool)
                        fx, fy = (np.where(np.isnan(v), np.nanmin(v) - 0.1, v)[keep] for v in (x, y))
                        r, s = np.triu_indices(len(fx), k=1)
                        conc = np.sign(fx[r] - fx[s]) * np.sign(fy[r] - fy[s])
                        assert int(conc.sum()) == d.num[a, b] and int(np.abs(conc).sum()) == d.plus(a, b)
                assert np.array_equal(d.key, d.key.T) and np.array_equal(np.sign(d.key), np.sign(d.num))
                order = np.argsort(d.key[d.valid], kind="stable")
                fr = [Fraction(int(p), int(q)) for p, q in zip(d.num[d.valid][order], d.den(*np.nonzero(d.valid))[order])]
                ks = d.key[d.valid][order]
                assert all((f1 < f2) == (k1 < k2) for f1, f2, k1, k2 in zip(fr, fr[1:], ks, ks[1:]))   # key orders the fractions


def _cens_classes(d):
    return gpu_base._classes(d, "interleaved")


def _oracle_plane(d, perspective, column=1, alternative="two.sided"):
    iu, ju = np.triu_indices(d.S, k=1)
    out = O.ici_pairs(d.X, iu.astype(np.int32), ju.astype(np.int32), perspective=perspective, alternative=alternative,
                      want_counts=False)[0]
    plane = np.full((d.S, d.S), np.nan)
    plane[iu, ju] = plane[ju, iu] = out[:, column]
    return plane


@pytest.mark.parametrize("perspective", ["global", "local"])
@pytest.mark.parametrize("key", CENS130)
def test_censored_entries_against_the_checkers(key, perspective):
    """every closed-form entry answer on the S = 130 censored designs against its brute-force checker fed the design's
    five matrices (the p-value plane is the CPU oracle's)"""
    d = _gpu_design(key).under(perspective)
    assert d.n <= 200 and d.distinct_doubles
    S = d.S
    pplane = _oracle_plane(d, perspective)
    cls, n_class = _cens_classes(d)
    same = cls[:, None] == cls[None, :]
    mx_all, mx_in = d.max_taumax(), d.max_taumax(same)
    assert np.array_equal(bits(_oracle_plane(d, perspective, 0)[d.valid]), bits(d.raw[d.valid]))
    assert np.array_equal(bits(_oracle_plane(d, perspective, 2)[d.valid]), bits(d.taumax(*np.nonzero(d.valid))))
    for scale_max in (True, False):
        m5 = d.planes(None, scale_max, pplane)
        rows = np.arange(S)[:, None]
        for k in (1, 7, S + 4):
            idx, _keys, raw, n_valid = dt.topk(d, k)
            ridx, rvals, rn = brute_topk(m5, k)
            assert np.array_equal(idx, ridx) and np.array_equal(n_valid, rn)
            want = dt.carried(d, rows, idx, mx_all, scale_max, pplane[rows, np.maximum(idx, 0)])
            assert np.array_equal(bits(want), bits(rvals)) and np.array_equal(bits(raw), bits(rvals[1]))
        cnt = dt.group_counts(d)[0][0]
        t = int(np.argmax(cnt)) - d.K                                      # the key most pairs equal
        comp = d.planes()[4]
        c0 = float(np.unique(comp[d.valid])[-2]) if len(np.unique(comp[d.valid])) > 1 else 1.0
        p0 = float(np.sort(pplane[d.valid])[int(d.valid.sum()) // 2])       # a value of the p plane itself
        for absolute in (False, True):
            for also, kw in ((None, {}), ((comp >= c0) & (pplane <= p0), {"min_completeness": c0, "max_pvalue": p0})):
                ei, ej, _keys, raw, n_edges, degree = dt.edges(d, t, absolute, also)
                rei, rej, rvals, rn, rdeg = brute_edges(m5, min_raw=float(d.value(t)), absolute=absolute, **kw)
                assert n_edges == rn > 0 and np.array_equal(ei, rei) and np.array_equal(ej, rej) and np.array_equal(degree, rdeg)
                assert np.array_equal(bits(dt.carried(d, ei, ej, mx_all, scale_max, pplane[ei, ej])), bits(rvals))
        for c, nc in ((None, 1), (cls, n_class)):
            cm = dt.class_matrix(d, c, nc)
            med2, n_valid = brute_class_matrix(m5, c, nc)
            assert np.array_equal(cm["n_valid"], n_valid) and np.array_equal(bits(cm["med"]), bits(med2[1]))
            assert np.array_equal(bits(dt.median_cor(d, cm, mx_all) if scale_max else cm["med"]), bits(med2[0]))
            own = dt.class_medians(d, c)
            rule = mx_all if c is None else mx_in                            # class_medians: the within-class pairs' maximum
            med2, n_valid = brute_medians(d.planes(None if c is None else same, scale_max), c)
            assert np.array_equal(own["n_valid"], n_valid) and np.array_equal(bits(own["med"]), bits(med2[1]))
            assert np.array_equal(bits(dt.median_cor(d, own, rule) if scale_max else own["med"]), bits(med2[0]))
        counts = dt.group_counts(d, cls)
        vals = np.nonzero(counts[0][0])[0] - d.K
        bn = vals[1:-1:3]
        q, order2, _ord, n_valid, n_na = dt.quantiles(d, PROBS, cls, counts)
        qc = dt.quantiles(d, PROBS, cls, counts, mx_all)[0] if scale_max else q
        hist, outside = dt.histogram(d, bn, cls, counts)
        rq2, rorder2, rnv, rna, rhist, rout = brute_quantiles(m5, cls, PROBS, d.value(bn))
        assert np.array_equal(hist, rhist) and np.array_equal(outside, rout) and np.array_equal(n_valid, rnv)
        assert np.array_equal(bits(order2), bits(rorder2)) and np.array_equal(bits(q), bits(rq2[1]))
        assert np.array_equal(bits(qc), bits(rq2[0]))
        # the rectangle: its own maximum, not the stacked triangle's
        for Sq in (5, 8):
            r = dt.rect(d, Sq)
            mx_r = r.max_taumax()
            mask = np.zeros((S, S), dtype=bool)
            mask[:Sq, Sq:] = True
            rect5 = np.ascontiguousarray(d.planes(mask, scale_max, pplane)[:, :Sq, Sq:])
            assert cross_checker.max_taumax(rect5) == mx_r
            for k in (1, 7, r.Sr):
                idx, _keys, topraw, n_valid = dt.cross_topk(d, Sq, k)
                ridx, rvals, rn = cross_checker.brute_cross_topk(rect5, k)
                assert np.array_equal(idx, ridx) and np.array_equal(n_valid, rn)
                qrows = np.arange(Sq)[:, None]
                want = dt.carried(d, qrows, np.where(idx >= 0, idx + Sq, -1), mx_r, scale_max, pplane[qrows, np.maximum(idx, 0) + Sq])
                assert np.array_equal(bits(want), bits(rvals))
            ref_cls = np.ascontiguousarray(gpu_base._classes(d, "na-class")[0][Sq:])
            cm = dt.cross_class_table(d, Sq, ref_cls, n_class)
            med2, n_valid = brute_cross_class(rect5, ref_cls, n_class)
            assert np.array_equal(cm["n_valid"], n_valid) and np.array_equal(bits(cm["med"]), bits(med2[1]))
            assert np.array_equal(bits(dt.median_cor(d, cm, mx_r) if scale_max else cm["med"]), bits(med2[0]))
    # the entries that take raw alone: ranks, quantised dissimilarities, sorted p-values, the forest
    perms = anosim_checker.documented_permutations(cls, 7, seed=11)
    got, want = dt.anosim(d, cls, n_class, perms), anosim_checker.brute_anosim(d.raw, cls, n_class, perms)
    for name in got:
        _same_item(got[name], want[name], name)
    for dd in (d, dt.valid_columns(d)):
        c2 = cls if dd is d else np.ascontiguousarray(cls[d.kind == dt.VALID])
        p2 = anosim_checker.documented_permutations(c2, 7, seed=11)
        got, want = dt.permanova(dd, c2, n_class, p2), permanova_checker.brute_permanova(dd.raw, c2, n_class, p2)
        for name in got:
            _same_item(got[name], want[name], name)
        from tests import permdisp_checker
        n_val, n_na, Q, T, A, sizes = dt.permdisp_table(dd, c2, n_class)
        assert (n_val, n_na, Q, T.tolist(), A, sizes) == permdisp_checker.brute_table(dd.raw, c2, n_class)
    for alternative, one_sided in (("two.sided", False), ("greater", True)):
        plane = _oracle_plane(d, perspective, 1, alternative)
        i, j, _k, n_na = dt.triangle(d)
        keys, count, fi, fj, _n = dt.pvalue_keys(d, one_sided)
        at = np.searchsorted(keys, d.pvalue_id(i, j, one_sided))
        assert np.array_equal(bits(plane[i, j]), bits(plane[fi, fj][at]))     # p is a function of (num, den, n_eff) alone
        p, got_na = dt.sorted_pvalues(d, plane[fi, fj], one_sided)
        want, want_na = padjust_checker.sorted_tests(np.where(np.triu(np.ones(plane.shape, dtype=bool), 1), plane, np.nan))
        assert got_na == want_na == n_na and np.array_equal(bits(p), bits(want))
    print(key, perspective, "max_taumax: all", mx_all, "within-class", mx_in, "rectangles", dt.rect(d, 5).max_taumax(),
          dt.rect(d, 8).max_taumax(), "distinct keys", d.K)


@pytest.mark.parametrize("key", CENS130)
def test_replayed_defects_show_on_the_censored_designs(key):
    """Five defects restated in numpy on the entry references (not the kernels); each must change the answer on every
    S = 130 censored design of the GPU files, under both perspectives.  Cells counted over: top-7 of every sample (cor by
    the all-pairs maximum), class_medians (the within-class maximum), class_matrix (all pairs) and the 8-query rectangle
    (its own maximum).  (d) cannot show on the ties-only variant, where nothing is missing and the perspectives agree:
    it is asserted to be 0 there."""
    d0 = _gpu_design(key)
    S, Sq = d0.S, 8
    cls, n_class = gpu_base._labels_that_split_the_maximum(d0) if key == "cens64-apart" else _cens_classes(d0)
    same = cls[:, None] == cls[None, :]
    rows = np.arange(S)[:, None]
    differ = lambda x, y: int(np.sum(bits(x) != bits(y)))               # noqa: E731
    for perspective in ("global", "local"):
        d, g = d0.under(perspective), d0.under("global")
        mx_all, mx_in = d.max_taumax(), d.max_taumax(same)
        idx = dt.topk(d, 7)[0]
        top = dt.carried(d, rows, idx, mx_all)
        own, cm = dt.class_medians(d, cls), dt.class_matrix(d, cls, n_class)
        r = dt.rect(d, Sq)
        mx_r = r.max_taumax()
        rraw = r.raw[r.valid]
        last = max(int(i) for i in np.nonzero(np.triu(d.valid, 1).any(axis=1))[0])      # a row per block: the last block
        mask = np.zeros((S, S), dtype=bool)
        mask[last, last + 1:] = True
        mx_last = d.max_taumax(mask)
        n = {
            "a": differ(top[0], top[1]) + differ(dt.median_cor(d, own, mx_in), own["med"])
                 + differ(dt.median_cor(d, cm, mx_all), cm["med"]) + differ(dt.cor_value(rraw, mx_r), rraw),
            "b": differ(dt.median_cor(d, own, mx_all), dt.median_cor(d, own, mx_in))
                 + differ(dt.median_cor(d, cm, mx_in), dt.median_cor(d, cm, mx_all))
                 + differ(dt.cor_value(rraw, mx_all), dt.cor_value(rraw, mx_r)),
            "c": differ(top[3], top[4]),
            "d": int(np.sum(dt.topk(g, 7)[0] != idx)) + differ(dt.carried(g, rows, idx, g.max_taumax()), top),
            "e": differ(dt.carried(d, rows, idx, mx_last)[0], top[0]) + differ(dt.median_cor(d, cm, mx_last), dt.median_cor(d, cm, mx_all)),
        }
        print(key, perspective, "cells that change under the replayed defects", n, "max_taumax all / within / rectangle / last block",
              mx_all, mx_in, mx_r, mx_last)
        assert n["a"] > 0 and n["b"] > 0 and n["c"] > 0 and n["e"] > 0
        if perspective == "local":
            assert (n["d"] > 0) == (key != "cens64-ties")
