"""The five selection entries (topk, edges, class_medians, class_matrix, quantiles) on designed matrices whose
ICI-Kendall-tau is known in closed form from integers (tests/designed_tau.py): the reference needs no S x S matrix from
the library and no oracle run, so it reaches the key space and the sizes that the entries' own test files cannot.

Every test first asserts that Context.pairs gives the closed form BITWISE on the first 2 000 combn pairs of its input
(_closed_form_pairs).  From there every float an entry returns -- raw, cor, taumax, medians, order statistics,
quantiles -- is compared bitwise with num / m, and every index, count and ordering with the integers.

The censored family (test_censored_*, at the end) has taumax, completeness and max_taumax below 1: there the
precondition also holds taumax, completeness and the counts, and every carried plane and cor's divisor is compared."""
import time

import numpy as np
import pytest

from icikendalltau_amd import _lib
from tests import designed_tau as dt
from tests.edges_checker import combn_pairs
from tests.quantiles_checker import PROBS
from tests.test_gpu_medians import _five_classes, _interleaved

pytestmark = pytest.mark.gpu

bits = dt.bits
NA = dt.NA_REAL_BITS
ONE = bits(np.array(1.0))[0]
CONFIGS = [("global", True), ("global", False), ("local", True), ("local", False)]
_DESIGN = {}
_PAIRS_OK = set()


# ---- the designs -----------------------------------------------------------------------------------------------------

def _two_valued(balance):
    """Every valid column is +-base, so raw is -1 or +1 and runs of thousands of equal keys sit at both ends of key
    space.  121 valid columns, 5 all-NaN and 4 constant ones.
    balance "classes": inside each interleaved class the signs are split evenly (an odd count: one more +), so a
    sample's cell of a class of even valid count -- and a + sample's cell of its own class of odd count -- has -1 and
    +1 as its middle keys.
    balance "all": 66 + and 55 - columns: 66 * 55 = 3 630 of the 7 260 valid pairs are -1, exactly half."""
    S, n = 130, 40
    probe = dt.swaps(S, n, seed=6, values=[0], n_all_missing=5, n_constant=4)
    good = np.nonzero(probe.kind == dt.VALID)[0]
    signs = np.ones(len(good), dtype=np.int32)
    if balance == "all":
        signs[np.random.default_rng(8).choice(len(good), size=55, replace=False)] = -1
    else:
        cls, n_class = _interleaved(S)
        for c in range(n_class):
            at = np.nonzero(cls[good] == c)[0]
            signs[at[(len(at) + 1) // 2:]] = -1
    return dt.swaps(S, n, seed=6, params=np.zeros(len(good), dtype=np.int64), signs=signs, n_all_missing=5, n_constant=4)


def _design(key):
    if key not in _DESIGN:
        _DESIGN[key] = {
            "two-valued": lambda: _two_valued("classes"),
            "two-valued-half": lambda: _two_valued("all"),
            "swaps40": lambda: dt.swaps(130, 40, seed=1, n_all_missing=2, n_constant=1),
            # five prefix lengths: 11 distinct |num|, each shared by hundreds of pairs
            "reversals41": lambda: dt.reversals(130, 41, seed=2, values=[0, 3, 9, 20, 41], n_all_missing=1, n_constant=2),
            # every prefix length: hundreds of distinct values, keys that differ from their top digits down
            "reversals41-wide": lambda: dt.reversals(130, 41, seed=2, n_all_missing=1, n_constant=2),
            "rev24-2049": lambda: dt.reversals(2049, 24, seed=3, n_all_missing=1, n_constant=1),
            "rev24-4098": lambda: dt.reversals(4098, 24, seed=4),
            "rev24-5794": lambda: dt.reversals(5794, 24, seed=5, n_all_missing=1, n_constant=1),
            # tied, left-censored columns (64 rows: a bottom block of 8 with 3 NaN, 28 adjacent pairs of which 5 are
            # tied).  No two columns alike but the first two valid ones: the one pair with taumax == 1, in the first block
            "cens64": lambda: dt.censored(130, 64, 8, 3, 5, seed=1, n_lib=6, max_overlap=1, n_all_missing=1, n_constant=1),
            "cens64-ties": lambda: dt.censored(130, 64, 8, 3, 5, seed=1, variant="ties", n_lib=6, max_overlap=1, n_all_missing=1, n_constant=1),
            # no two columns alike at all: every taumax is below 1, so cor != raw under every entry's rule
            "cens64-apart": lambda: dt.censored(130, 64, 8, 3, 5, seed=2, own_state=True, twin=False, n_all_missing=2, n_constant=1),
            "cens64-2049": lambda: dt.censored(2049, 64, 8, 3, 5, seed=3, n_lib=56, n_all_missing=1, n_constant=1),
        }[key]()
    return _DESIGN[key]


def _closed_form_pairs(ctx, key, perspectives=("global", "local")):
    """Context.pairs == the closed form, bitwise, on the first 2 000 combn pairs: what every assertion below rests on"""
    d = _design(key)
    for perspective in perspectives:
        if (key, perspective) in _PAIRS_OK:
            continue
        pi, pj = combn_pairs(d.S)
        pi, pj = pi[:2000], pj[:2000]
        if isinstance(d, dt.Censored):
            _censored_pairs(ctx, d.under(perspective), key, perspective, pi, pj)
            _PAIRS_OK.add((key, perspective))
            continue
        out, _cnt, rsn = ctx.pairs(d.X, pi, pj, perspective=perspective, want_counts=False)
        ok = d.valid[pi, pj]
        want = d.value(d.num[pi, pj])
        diff = np.nonzero(bits(out[ok, 0]) != bits(want[ok]))[0]
        print(key, perspective, "pairs checked", len(pi), "valid", int(ok.sum()), "raw differs on", len(diff),
              [(hex(int(a)), hex(int(b))) for a, b in zip(bits(out[ok, 0])[diff[:5]], bits(want[ok])[diff[:5]])])
        assert np.array_equal(rsn, d.reasons()[pi, pj])
        assert len(diff) == 0
        assert np.all(bits(out[ok, 2]) == ONE) and np.all(bits(out[ok, 3]) == ONE)      # taumax, completeness
        assert np.all(np.isnan(out[~ok]))
        _PAIRS_OK.add((key, perspective))
    return d


def _censored_pairs(ctx, dv, key, perspective, pi, pj):
    """the precondition on the censored family: raw and taumax bitwise, the eleven counts and the reasons exact,
    completeness bitwise the float64 expression 1.0 - missing / n_eff and within 1 ulp of the fraction, the p-value
    within the device bound of tests/epilogue_checker.check_call (4 E_CPU) of the exact epilogue on the design's counts"""
    from fractions import Fraction
    from tests import epilogue_checker as E
    out, cnt, rsn = ctx.pairs(dv.X, pi, pj, perspective=perspective)
    ok = dv.valid[pi, pj]
    a, b = pi[ok], pj[ok]
    counts = dv.counts(a, b)
    diff = {name: int(np.sum(bits(out[ok, col]) != bits(want))) for name, col, want in
            (("raw", 0, dv.raw[a, b]), ("taumax", 2, dv.taumax(a, b)), ("completeness", 3, dv.completeness(a, b)))}
    bad_counts = int(np.sum((cnt[ok][:, :11] != counts).any(axis=1)))
    first = np.nonzero(bits(out[ok, 0]) != bits(dv.raw[a, b]))[0][:3]
    print(key, perspective, "pairs checked", len(pi), "valid", int(ok.sum()), "bits that differ", diff, "count records", bad_counts,
          [(int(dv.num[a[q], b[q]]), int(dv.den(a[q], b[q])), float(out[ok, 0][q]).hex()) for q in first])
    assert np.array_equal(rsn, dv.reasons()[pi, pj]) and np.all(np.isnan(out[~ok]))
    assert bad_counts == 0
    assert diff["raw"] == 0 and diff["taumax"] == 0 and diff["completeness"] == 0
    miss, ne = dv.missing(a, b), dv.n_eff(a, b)
    for g, m_, e in set(zip(out[ok, 3].tolist(), miss.tolist(), ne.tolist())):
        exact = Fraction(e - m_, e)
        assert abs(Fraction(g) - exact) <= Fraction(float(np.spacing(float(exact))))
    worst = E.check_call(out[ok], counts, "two.sided", False, 4 * E.E_CPU["cases"], f"{key} {perspective}")
    print(key, perspective, "worst scaled p error", worst["p"])


def _p_of(ctx, dv, perspective):
    """p(a, b) for index arrays of valid pairs: one Context.pairs p-value per distinct (|num|, den, n_eff) of the design,
    looked up per pair -- the p-value has no closed form"""
    cache = dv.__dict__.setdefault("_p_table", {})
    if perspective not in cache:
        keys, _count, fi, fj, _n_na = dt.pvalue_keys(dv)
        cache[perspective] = keys, _pvalues(ctx, dv, fi, fj, perspective)
    keys, p = cache[perspective]

    def look(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return p[np.searchsorted(keys, dv.pvalue_id(np.minimum(a, b), np.maximum(a, b)))]
    return look


def _labels_that_split_the_maximum(d0):
    """two classes such that every pair at the largest taumax, under either perspective, lies across them: the
    within-class maximum is then strictly below the all-pairs one (a 2-colouring of those few pairs)"""
    S = d0.S
    near = [[] for _ in range(S)]
    for perspective in ("global", "local"):
        d = d0.under(perspective)
        a, b = np.nonzero(np.triu(d.valid, 1))
        tm = d.taumax(a, b)
        for x, y in zip(a[tm == tm.max()], b[tm == tm.max()]):
            near[x].append(int(y))
            near[y].append(int(x))
    colour = np.full(S, -1, dtype=np.int32)
    for s in range(S):
        if colour[s] >= 0:
            continue
        colour[s] = s % 2 if not near[s] else 0
        todo = [s]
        while todo:
            x = todo.pop()
            for y in near[x]:
                assert colour[y] != colour[x], "the pairs at the maximum have an odd cycle"
                if colour[y] < 0:
                    colour[y] = 1 - colour[x]
                    todo.append(y)
    return colour, 2


def _classes(d, kind):
    """"interleaved": classes of 1, 2, 3, 60 and 64 samples, class index 2 empty; "na-class": the same with the NA
    columns moved into class 2, a class of NA columns alone"""
    cls, n_class = _interleaved(d.S)
    if kind == "na-class":
        cls = cls.copy()
        cls[d.kind != dt.VALID] = 2
    return cls, n_class


def _rc5(d, cls=None):
    """reason_counts over all pairs, or with cls over the within-class pairs"""
    if cls is None:
        return d.reason_counts()
    iu, ju = np.triu_indices(d.S, k=1)
    same = cls[iu] == cls[ju]
    return np.bincount(d.reasons()[iu, ju][same], minlength=5).astype(np.int64)


def _pvalues(ctx, d, a, b, perspective="global"):
    """the p-value plane has no closed form here: the pair kernel's own, asked for the same pairs"""
    lo, hi = np.minimum(a, b).astype(np.int32), np.maximum(a, b).astype(np.int32)
    out, _cnt, _rsn = ctx.pairs(d.X, lo, hi, perspective=perspective, want_counts=False)
    return out[:, 1]


# ---- medians: class_matrix and class_medians -------------------------------------------------------------------------

def _assert_class_matrix(got, d, cm):
    med2, n_valid, mx, rc5 = got
    print("cells differing", int(np.sum(bits(med2[1]) != bits(cm["med"]))), int(np.sum(bits(med2[0]) != bits(cm["med"]))))
    assert np.array_equal(n_valid, cm["n_valid"])
    assert np.array_equal(bits(med2[1]), bits(cm["med"]))
    assert np.array_equal(bits(med2[0]), bits(cm["med"]))          # taumax == 1: cor is raw
    assert mx == d.max_taumax() and np.array_equal(rc5, d.reason_counts())


@pytest.mark.parametrize("classes", ["interleaved", "na-class"])
@pytest.mark.parametrize("key", ["two-valued", "swaps40", "reversals41", "reversals41-wide"])
def test_class_matrix(hip_ctx, key, classes):
    d = _closed_form_pairs(hip_ctx, key)
    cls, n_class = _classes(d, classes)
    cm = dt.class_matrix(d, cls, n_class)
    have, even = cm["n_valid"] > 0, cm["n_valid"] % 2 == 0
    zero = have & even & (cm["lo"] == -cm["hi"]) & (cm["lo"] != 0)
    edge = have & even & (cm["k_in"] + 1 == cm["run"])
    inside = have & even & (cm["k_in"] + 1 < cm["run"])
    print(key, classes, "cells: -x/+x", int(zero.sum()), "edge of a run", int(edge.sum()), "inside a run", int(inside.sum()))
    assert edge.any() and inside.any()
    if key == "two-valued":
        assert zero.sum() >= 100 and np.all(cm["lo"][zero] == -d.m) and cm["run"][zero].max() >= 30
        assert np.all(bits(cm["med"][zero]) == 0)                  # the reference itself says +0.0
    if classes == "na-class":
        assert np.all(cm["n_valid"][:, 2] == 0) and np.all(bits(cm["med"][:, 2]) == NA)
    outs = []
    for perspective, scale_max in CONFIGS:
        got = hip_ctx.class_matrix(d.X, cls, n_class, None, perspective, "two.sided", False, 0, scale_max)
        _assert_class_matrix(got, d, cm)
        assert np.all(bits(got[0][:, zero]) == 0)                  # +0.0, through mean2 and plus_zero
        outs.append(got)
    for got in outs[1:]:
        assert np.array_equal(bits(got[0]), bits(outs[0][0]))


@pytest.mark.parametrize("classes", ["one", "interleaved", "na-class"])
@pytest.mark.parametrize("key", ["two-valued", "swaps40", "reversals41", "reversals41-wide"])
def test_class_medians(hip_ctx, key, classes):
    d = _closed_form_pairs(hip_ctx, key)
    cls, n_class = (None, 1) if classes == "one" else _classes(d, classes)
    own = dt.class_medians(d, cls)
    have, even = own["n_valid"] > 0, own["n_valid"] % 2 == 0
    zero = have & even & (own["lo"] == -own["hi"]) & (own["lo"] != 0)
    print(key, classes, "samples: -x/+x", int(zero.sum()), "edge", int((have & even & (own["k_in"] + 1 == own["run"])).sum()))
    if key == "two-valued" and classes != "one":
        assert zero.sum() >= 30 and np.all(bits(own["med"][zero]) == 0)
    within = _rc5(d, np.zeros(d.S, dtype=np.int32) if cls is None else cls)
    for perspective, scale_max in CONFIGS:
        med2, n_valid, mx, rc5 = hip_ctx.class_medians(d.X, cls, n_class, None, perspective, "two.sided", False, 0, scale_max)
        assert np.array_equal(n_valid, own["n_valid"])
        assert np.array_equal(bits(med2[1]), bits(own["med"])) and np.array_equal(bits(med2[0]), bits(own["med"]))
        assert np.all(bits(med2[:, zero]) == 0)
        assert mx == (1.0 if within[0] else -np.inf) and np.array_equal(rc5, within)
    if classes == "na-class":
        assert np.all(n_valid[d.kind != dt.VALID] == 0) and np.all(bits(med2[:, d.kind != dt.VALID]) == NA)


# ---- top-k -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["two-valued", "swaps40", "reversals41"])
def test_topk_with_ties_at_the_kth_place(hip_ctx, key):
    d = _closed_form_pairs(hip_ctx, key)
    S = d.S
    good = d.kind == dt.VALID
    for k in (1, 7, 129, 256):
        idx, nums, raw, n_valid = dt.topk(d, k)
        if k <= 7:   # samples whose k-th value is shared by partners beyond the k-th place: the index alone decides
            kth = nums[:, k - 1]
            tied = good & ((d.valid & (d.num >= kth[:, None])).sum(axis=1) > k)
            print(key, "k", k, "samples with a tie across the k-th place", int(tied.sum()))
            assert tied.sum() >= (100 if key == "two-valued" else 10)
        else:
            assert np.all(n_valid == d.valid.sum(axis=1)) and np.all(idx[:, n_valid.max():] == -1)
        for perspective, scale_max in (CONFIGS if k == 7 else CONFIGS[:1]):
            gidx, vals, gn, mx, rc5 = hip_ctx.topk(d.X, k, None, perspective, "two.sided", False, 0, scale_max)
            assert np.array_equal(gn, n_valid) and np.array_equal(gidx, idx)
            assert np.array_equal(bits(vals[1]), bits(raw)) and np.array_equal(bits(vals[0]), bits(raw))
            assert np.all(bits(vals[3:5])[:, idx >= 0] == ONE) and np.all(bits(vals)[:, idx < 0] == NA)
            assert mx == 1.0 and np.array_equal(rc5, d.reason_counts())
            if k == 7:
                rows = np.repeat(np.arange(S), k).reshape(S, k)
                sel = idx >= 0
                assert np.array_equal(bits(vals[2][sel]), bits(_pvalues(hip_ctx, d, rows[sel], idx[sel], perspective)))


# ---- edges -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["two-valued", "swaps40", "reversals41"])
def test_edges_at_a_threshold_that_hundreds_of_pairs_equal(hip_ctx, key):
    d = _closed_form_pairs(hip_ctx, key)
    cnt = dt.group_counts(d)[0][0]
    both = cnt + cnt[::-1]                                            # pairs per |num|
    t = int(np.max(np.nonzero((cnt >= 200) & (cnt[::-1] >= 200))[0])) - d.m     # the largest value that 200 pairs equal, with either sign
    assert t > 0 and cnt[t + d.m] >= 200 and cnt[-t + d.m] >= 200 and both[t + d.m] >= 400
    min_raw = float(d.value(t))
    print(key, "threshold", t, "/", d.m, "pairs equal to it", int(cnt[t + d.m]), "to its negative", int(cnt[-t + d.m]))
    for absolute in (False, True):
        ei, ej, nums, raw, n_edges, degree = dt.edges(d, t, absolute)
        above = dt.edges(d, t + 1, absolute)[4]
        assert n_edges - above == (both if absolute else cnt)[t + d.m]            # the pairs that sit ON the bound
        for perspective, scale_max in CONFIGS:
            for room in (n_edges, n_edges // 3, 0):
                gi, gj, vals, gn, gdeg, mx, rc5 = hip_ctx.edges(d.X, min_raw, None, None, absolute, room, None, perspective,
                                                               "two.sided", False, 0, scale_max)
                assert gn == n_edges and np.array_equal(gdeg, degree)
                assert np.array_equal(gi, ei[:room]) and np.array_equal(gj, ej[:room])
                assert np.array_equal(bits(vals[1]), bits(raw[:room])) and np.array_equal(bits(vals[0]), bits(raw[:room]))
                assert np.all(bits(vals[3:5]) == ONE)
                assert mx == 1.0 and np.array_equal(rc5, d.reason_counts())
        full = hip_ctx.edges(d.X, min_raw, None, None, absolute, n_edges)
        assert np.array_equal(bits(full[2][2]), bits(_pvalues(hip_ctx, d, ei, ej)))


# ---- quantiles and histogram -----------------------------------------------------------------------------------------

def _assert_quantiles(got, d, cls, probs, break_nums, counts=None):
    counts = dt.group_counts(d, cls) if counts is None else counts
    q2, order2, n_valid, n_na, hist, outside, mx, rc5 = got
    assert np.array_equal(n_valid, counts[1]) and np.array_equal(n_na, counts[2])
    if break_nums is not None:
        rh, ro = dt.histogram(d, break_nums, cls, counts)
        print("outside", outside.tolist(), "last bin", hist[:, -1].tolist())
        assert np.array_equal(hist, rh) and np.array_equal(outside, ro)
        assert np.array_equal(hist.sum(axis=1) + outside.sum(axis=1), n_valid)
    if len(probs):
        rq, rorder2, _ord_num, _nv, _na = dt.quantiles(d, probs, cls, counts)
        assert np.array_equal(bits(order2), bits(rorder2))
        assert np.array_equal(bits(q2[1]), bits(rq)) and np.array_equal(bits(q2[0]), bits(rq))
    assert mx == d.max_taumax() and np.array_equal(rc5, d.reason_counts())
    assert rc5.sum() == d.S * (d.S - 1) // 2 and n_valid[0] == rc5[0]


@pytest.mark.parametrize("classes", ["interleaved", "na-class"])
@pytest.mark.parametrize("key", ["two-valued", "two-valued-half", "swaps40", "reversals41", "reversals41-wide"])
def test_quantiles(hip_ctx, key, classes):
    d = _closed_form_pairs(hip_ctx, key)
    cls, n_class = _classes(d, classes)
    counts = dt.group_counts(d, cls)
    _rq, _ro, ord_num, n_valid, _n_na = dt.quantiles(d, PROBS, cls, counts)
    if key == "two-valued-half":     # group 0: 7 260 valid pairs, 3 630 of them -1: the median lies between -1 and +1
        assert n_valid[0] == 7260 and counts[0][0][0] == 3630 and ord_num[0][2].tolist() == [-d.m, d.m]
    outs = []
    for perspective, scale_max in CONFIGS:
        for c, nc in ((cls, n_class), (None, 1)):
            got = hip_ctx.quantiles(d.X, PROBS, None, c, nc, None, perspective, "two.sided", False, 0, scale_max)
            _assert_quantiles(got, d, c, PROBS, None, counts if c is not None else None)
            if key == "two-valued-half":
                assert bits(got[0][:, 0, 2]).tolist() == [0, 0] and got[1][0, 2].tolist() == [-1.0, 1.0]
        outs.append(got)
    for got in outs[1:]:
        assert np.array_equal(bits(got[0]), bits(outs[0][0]))


def _break_sets(d, counts):
    """break numerators by case, taken from the design's own values so that values sit exactly on breaks"""
    cnt = counts[0][0]
    vals = np.nonzero(cnt)[0] - d.m                                   # the distinct numerators of all pairs, ascending
    sets = {"two": np.array([vals[1], vals[-2]]) if len(vals) > 3 else np.array([-d.m + 2, d.m - 2])}
    # first break on the minimum, last break ON the maximum: nothing outside, the last bin closed on the right
    sets["last-on-max"] = np.unique(np.concatenate([vals[:1], vals[2:-1:3], vals[-1:]]))
    # an interior break on a run of equal non-zero values
    run = int(vals[np.argmax(np.where((vals != 0) & (vals > vals[0]) & (vals < vals[-1]), cnt[vals + d.m], -1))]) \
        if len(vals) > 2 else 0
    sets["interior-on-run"] = np.array([vals[0], run, vals[-1]])
    # strictly inside the data's range: values below the first and above the last break
    sets["inside"] = vals[2:-2:2] if len(vals) > 8 else np.array([-1, 1])
    # ICIKT_HIST_MAX_BINS bins, the last break on m
    sets["1025"] = d.m - 2 * np.arange(1024, -1, -1)
    return vals, cnt, sets


@pytest.mark.parametrize("case", ["two", "last-on-max", "interior-on-run", "inside", "1025"])
@pytest.mark.parametrize("key", ["two-valued", "swaps40", "reversals41"])
def test_histogram_breaks_on_values(plan_ctx, key, case):
    d = _closed_form_pairs(plan_ctx, key, ("global",))
    cls, n_class = _classes(d, "interleaved")
    counts = dt.group_counts(d, cls)
    vals, cnt, sets = _break_sets(d, counts)
    bn = sets[case]
    breaks = d.value(bn)
    rh, ro = dt.histogram(d, bn, cls, counts)
    assert len(bn) >= 2 and np.all(np.diff(bn) > 0)
    if case in ("last-on-max", "interior-on-run", "1025"):
        assert bn[-1] == vals[-1] == d.m and np.all(ro == 0)
        assert cnt[2 * d.m] > 0 and rh[0, -1] >= cnt[2 * d.m]          # the maximum is counted in the last bin
    if case == "interior-on-run" and key != "two-valued":
        assert bn[1] != 0 and cnt[bn[1] + d.m] >= 100 and rh[0, 1] >= cnt[bn[1] + d.m]
    if case == "inside":
        assert np.all(ro > 0)                                          # below and above, in all three groups
    if case == "1025":
        assert len(bn) == _lib.HIST_MAX_BINS + 1
    for spec in ((None, "tkblock=1") if case == "1025" else (None,)):
        plan_ctx.debug_set_plan(spec)
        got = plan_ctx.quantiles(d.X, (0.5, 0.0, 1.0), breaks, cls, n_class)
        _assert_quantiles(got, d, cls, (0.5, 0.0, 1.0), bn, counts)
        one = plan_ctx.quantiles(d.X, (), breaks)
        _assert_quantiles(one, d, None, (), bn)


# ---- sizes past the thresholds (prefix reversals, n = 24) ------------------------------------------------------------

def _timed(label, fn):
    t0 = time.perf_counter()
    out = fn()
    print("TIME %s %.3f s" % (label, time.perf_counter() - t0))
    return out


def test_2049_samples_quantiles(hip_ctx):
    """2 098 176 pairs: more than 2 048 workgroups x 1 024 pairs, so k_quant_count's four-tile loop runs a second trip
    and steps its (row, place) across trips"""
    d = _closed_form_pairs(hip_ctx, "rev24-2049", ("global",))
    assert d.S * (d.S - 1) // 2 > 2048 * 1024
    cls, n_class = _five_classes(d.S)
    bn = np.arange(-300, 301, 3)
    assert len(bn) == 201 and bn[0] < -d.m and bn[-1] > d.m
    got = _timed("S=2049 quantiles", lambda: hip_ctx.quantiles(d.X, PROBS, d.value(bn), cls, n_class))
    _assert_quantiles(got, d, cls, PROBS, bn)


def test_2049_samples_edges(hip_ctx):
    """the bound is the largest value, raw == 1: with 24 rows the family has 24 distinct discordance counts and two
    signs, so no bound keeps fewer than 2 % of the pairs"""
    d = _closed_form_pairs(hip_ctx, "rev24-2049", ("global",))
    ei, ej, _nums, raw, n_edges, degree = dt.edges(d, d.m)
    total = d.S * (d.S - 1) // 2
    print("edges", n_edges, "of", total)
    assert 0.01 * total < n_edges < 0.03 * total
    gi, gj, vals, gn, gdeg, mx, rc5 = _timed("S=2049 edges", lambda: hip_ctx.edges(d.X, 1.0, max_edges=n_edges))
    assert gn == n_edges and np.array_equal(gdeg, degree) and np.array_equal(gi, ei) and np.array_equal(gj, ej)
    assert np.all(bits(vals[[0, 1, 3, 4]]) == ONE) and mx == 1.0 and np.array_equal(rc5, d.reason_counts())


def test_2049_samples_topk(hip_ctx):
    d = _closed_form_pairs(hip_ctx, "rev24-2049", ("global",))
    idx, _nums, raw, n_valid = dt.topk(d, 5)
    gidx, vals, gn, mx, rc5 = _timed("S=2049 topk", lambda: hip_ctx.topk(d.X, 5))
    assert np.array_equal(gn, n_valid) and np.array_equal(gidx, idx)
    assert np.array_equal(bits(vals[1]), bits(raw)) and np.array_equal(bits(vals[0]), bits(raw))
    assert mx == 1.0 and np.array_equal(rc5, d.reason_counts())


def _no_plan_override(monkeypatch):
    """the tests that override the plan restore it when they end (plan_ctx); these run under the natural plan and
    must not touch it"""
    def refuse(self, spec=None):
        raise AssertionError("debug_set_plan called in a test of the natural plan")
    monkeypatch.setattr(_lib.Context, "debug_set_plan", refuse)


def test_4098_samples_medians_reread_their_keys(hip_ctx, monkeypatch):
    """one class of 4 098 samples: 4 097 partners per cell, more than MEDIAN_STAGE_MAX = 4 096, so k_median_select and
    k_class_select re-read the kept plane in every pass under the natural plan; two classes of 4 097 and 1: the cells of
    4 096 partners are the largest that still stage, those of 4 097 re-read, in one launch"""
    _no_plan_override(monkeypatch)
    d = _closed_form_pairs(hip_ctx, "rev24-4098", ("global",))
    S = d.S
    assert S - 1 > 4096
    cm = dt.class_matrix(d)
    med2, n_valid, mx, rc5 = _timed("S=4098 class_medians", lambda: hip_ctx.class_medians(d.X))
    assert np.all(n_valid == S - 1) and np.array_equal(n_valid, cm["n_valid"][:, 0])
    assert np.array_equal(bits(med2[1]), bits(cm["med"][:, 0])) and np.array_equal(bits(med2[0]), bits(cm["med"][:, 0]))
    assert mx == 1.0 and np.array_equal(rc5, d.reason_counts())
    _assert_class_matrix(_timed("S=4098 class_matrix, one class", lambda: hip_ctx.class_matrix(d.X)), d, cm)
    cls = np.zeros(S, dtype=np.int32)
    cls[1234] = 1
    cm2 = dt.class_matrix(d, cls, 2)
    assert sorted(np.unique(cm2["n_valid"]).tolist()) == [0, 1, 4096, 4097]
    _assert_class_matrix(_timed("S=4098 class_matrix, classes of 4097 and 1", lambda: hip_ctx.class_matrix(d.X, cls, 2)), d, cm2)


def test_5794_samples_cut_the_triangle(hip_ctx, monkeypatch):
    """16 782 321 pairs, more than kTriangleBlockPairs = 2^24: the driver cuts the triangle into two blocks by itself"""
    _no_plan_override(monkeypatch)
    d = _closed_form_pairs(hip_ctx, "rev24-5794", ("global",))
    S = d.S
    total = S * (S - 1) // 2
    assert total > 1 << 24 and (S - 1) * (S - 2) // 2 <= 1 << 24
    bn = np.array([-d.m, -200, -90, 0, 50, 180, d.m])
    probs = (0.5, 0.01, 0.999)
    got = _timed("S=5794 quantiles", lambda: hip_ctx.quantiles(d.X, probs, d.value(bn)))
    _assert_quantiles(got, d, None, probs, bn)
    t = 200
    _ei, _ej, _nums, _raw, n_edges, degree = dt.edges(d, t)
    gi, gj, vals, gn, gdeg, mx, rc5 = _timed("S=5794 edges", lambda: hip_ctx.edges(d.X, float(d.value(t)), max_edges=0))
    assert gn == n_edges and np.array_equal(gdeg, degree) and len(gi) == 0
    assert mx == 1.0 and np.array_equal(rc5, d.reason_counts()) and rc5.sum() == total
    got = _timed("S=5794 class_matrix", lambda: hip_ctx.class_matrix(d.X))
    _assert_class_matrix(got, d, dt.class_matrix(d))
    assert got[3].sum() == total


# ---- the censored family: taumax, completeness and cor differ from each other, from raw and from 1 ---------------------

CENS130 = ["cens64", "cens64-ties", "cens64-apart"]


@pytest.mark.parametrize("spec", ["tkblock=1", "tkblock=4200"])
@pytest.mark.parametrize("key", CENS130)
def test_censored_selection_entries(plan_ctx, key, spec):
    """topk, edges, class_medians, class_matrix and quantiles on tied, left-censored columns: every carried plane bitwise
    (cor by the entry's own divisor, taumax and completeness each in its place), under a row per block and under a
    triangle cut in the middle (8 385 pairs in blocks of at most 4 200)"""
    ctx = plan_ctx
    d0 = _closed_form_pairs(ctx, key)
    S = d0.S
    cls, n_class = _classes(d0, "interleaved")
    same = cls[:, None] == cls[None, :]
    rows = np.arange(S)[:, None]
    ctx.debug_set_plan(spec)
    seen = {}
    for perspective, scale_max in CONFIGS:
        d = d0.under(perspective)
        p_of = _p_of(ctx, d, perspective)
        tail = (None, perspective, "two.sided", False, 0, scale_max)
        mx_all, mx_in, rc5 = d.max_taumax(), d.max_taumax(same), d.reason_counts()
        # top-k
        k = 7
        idx, keys, _raw, n_valid = dt.topk(d, k)
        tied = (d.valid & (d.key >= keys[:, k - 1][:, None])).sum(axis=1) > k
        gidx, vals, gn, mx, grc = ctx.topk(d.X, k, *tail)
        want = dt.carried(d, rows, idx, mx_all, scale_max, p_of(np.broadcast_to(rows, idx.shape), np.maximum(idx, 0)))
        print(key, spec, perspective, scale_max, "topk: tied across the k-th", int(tied.sum()), "planes differing",
              [int(np.sum(bits(vals[q]) != bits(want[q]))) for q in range(5)], "max_taumax", mx, mx_all, mx_in)
        assert tied.sum() >= 10 and np.array_equal(gidx, idx) and np.array_equal(gn, n_valid)
        assert np.array_equal(bits(vals), bits(want)) and mx == mx_all and np.array_equal(grc, rc5)
        seen[(perspective, scale_max)] = vals[0].copy()
        # edges: the key most pairs equal, a completeness many pairs equal, a p-value of the table
        cnt = dt.group_counts(d)[0][0]
        t = int(np.argmax(cnt)) - d.K
        a, b = np.nonzero(d.valid)
        comp, pp = np.full((S, S), np.nan), np.full((S, S), np.nan)
        comp[a, b], pp[a, b] = d.completeness(a, b), p_of(a, b)
        cvals, ccnt = np.unique(comp[a, b], return_counts=True)
        c0 = float(cvals[np.argmax(ccnt)])
        p0 = float(np.sort(pp[a, b])[len(a) // 2])                         # a value of the p table itself
        for also, bounds in ((None, (None, None)), ((comp >= c0) & (pp <= p0), (p0, c0))):
            for absolute in (False, True):
                ei, ej, _k, _r, n_edges, degree = dt.edges(d, t, absolute, also)
                gi, gj, vals, gn, gdeg, mx, grc = ctx.edges(d.X, float(d.value(t)), bounds[0], bounds[1], absolute, n_edges, *tail)
                assert gn == n_edges > 0 and np.array_equal(gi, ei) and np.array_equal(gj, ej) and np.array_equal(gdeg, degree)
                assert np.array_equal(bits(vals), bits(dt.carried(d, ei, ej, mx_all, scale_max, p_of(ei, ej))))
                assert mx == mx_all and np.array_equal(grc, rc5)
        on_bounds = int(np.sum(d.valid & (comp == c0))) // 2, int(np.sum(d.valid & (pp == p0))) // 2
        print("edges: pairs on the key", int(cnt[t + d.K]), "on min_completeness", on_bounds[0], "on max_pvalue", on_bounds[1])
        assert cnt[t + d.K] >= 100 and on_bounds[0] >= 100 and on_bounds[1] >= 1
        # medians: class_medians scales by the within-class pairs' maximum, class_matrix by all pairs', on the same labels
        own, cm = dt.class_medians(d, cls), dt.class_matrix(d, cls, n_class)
        med2, gn, mx, grc = ctx.class_medians(d.X, cls, n_class, *tail)
        assert np.array_equal(gn, own["n_valid"]) and np.array_equal(bits(med2[1]), bits(own["med"]))
        assert np.array_equal(bits(med2[0]), bits(dt.median_cor(d, own, mx_in) if scale_max else own["med"]))
        assert mx == mx_in and np.array_equal(grc, _rc5(d, cls))
        med2, gn, mx, grc = ctx.class_matrix(d.X, cls, n_class, *tail)
        assert np.array_equal(gn, cm["n_valid"]) and np.array_equal(bits(med2[1]), bits(cm["med"]))
        assert np.array_equal(bits(med2[0]), bits(dt.median_cor(d, cm, mx_all) if scale_max else cm["med"]))
        assert mx == mx_all and np.array_equal(grc, rc5)
        # quantiles and histogram
        counts = dt.group_counts(d, cls)
        bn = (np.nonzero(counts[0][0])[0] - d.K)[1:-1:3]
        q, order2, _o, nv, nna = dt.quantiles(d, PROBS, cls, counts)
        qc = dt.quantiles(d, PROBS, cls, counts, mx_all)[0] if scale_max else q
        hist, outside = dt.histogram(d, bn, cls, counts)
        q2, go2, gnv, gna, gh, gout, mx, grc = ctx.quantiles(d.X, PROBS, d.value(bn), cls, n_class, *tail)
        assert np.array_equal(gnv, nv) and np.array_equal(gna, nna) and np.array_equal(gh, hist) and np.array_equal(gout, outside)
        assert np.array_equal(bits(go2), bits(order2)) and np.array_equal(bits(q2[1]), bits(q)) and np.array_equal(bits(q2[0]), bits(qc))
        assert mx == mx_all and np.array_equal(grc, rc5)
        if key == "cens64-apart":            # labels under which the two rules differ on this design too
            cls2, n2 = _labels_that_split_the_maximum(d0)
            in2 = d.max_taumax(cls2[:, None] == cls2[None, :])
            assert in2 < mx_all
            own, cm = dt.class_medians(d, cls2), dt.class_matrix(d, cls2, n2)
            med2, gn, mx, grc = ctx.class_medians(d.X, cls2, n2, *tail)
            assert mx == in2 and np.array_equal(bits(med2[1]), bits(own["med"]))
            assert np.array_equal(bits(med2[0]), bits(dt.median_cor(d, own, in2) if scale_max else own["med"]))
            med2, gn, mx, grc = ctx.class_matrix(d.X, cls2, n2, *tail)
            assert mx == mx_all and np.array_equal(bits(med2[1]), bits(cm["med"]))
            assert np.array_equal(bits(med2[0]), bits(dt.median_cor(d, cm, mx_all) if scale_max else cm["med"]))
    dg = d0.under("global")
    if key in ("cens64", "cens64-ties"):     # the one pair with taumax == 1 lies across two classes, in the first block
        assert dg.max_taumax() == 1.0 > dg.max_taumax(same) and dg.taumax(0, 1) == 1.0
    if key == "cens64-apart":                # every taumax below 1: scale_max changes cor under every rule
        assert dg.max_taumax() < 1.0 and not np.array_equal(bits(seen[("global", True)]), bits(seen[("global", False)]))
        assert not np.array_equal(bits(seen[("local", True)]), bits(seen[("local", False)]))
    if key != "cens64-ties":                 # the perspectives differ
        assert not np.array_equal(bits(seen[("global", False)]), bits(seen[("local", False)]))


def test_2049_samples_censored_topk_and_edges(hip_ctx):
    """2 098 176 pairs of censored columns under the natural plan, global"""
    d = _closed_form_pairs(hip_ctx, "cens64-2049", ("global",))
    p_of = _p_of(hip_ctx, d, "global")
    rows = np.arange(d.S)[:, None]
    mx_all = d.max_taumax()
    idx, _k, _r, n_valid = _timed("S=2049 censored topk, the reference", lambda: dt.topk(d, 5))
    gidx, vals, gn, mx, rc5 = _timed("S=2049 censored topk", lambda: hip_ctx.topk(d.X, 5))
    assert np.array_equal(gidx, idx) and np.array_equal(gn, n_valid) and mx == mx_all == 1.0
    want = dt.carried(d, rows, idx, mx_all, True, p_of(np.broadcast_to(rows, idx.shape), np.maximum(idx, 0)))
    assert np.array_equal(bits(vals), bits(want)) and np.array_equal(rc5, d.reason_counts())
    t = d.K - 3
    ei, ej, _k, _r, n_edges, degree = _timed("S=2049 censored edges, the reference", lambda: dt.edges(d, t))
    gi, gj, vals, gn, gdeg, mx, rc5 = _timed("S=2049 censored edges", lambda: hip_ctx.edges(d.X, float(d.value(t)), max_edges=n_edges))
    print("edges", n_edges)
    assert gn == n_edges > 100 and np.array_equal(gi, ei) and np.array_equal(gj, ej) and np.array_equal(gdeg, degree)
    assert np.array_equal(bits(vals), bits(dt.carried(d, ei, ej, mx_all, True, p_of(ei, ej)))) and mx == mx_all


def test_2049_samples_censored_quantiles(hip_ctx):
    """the second trip of k_quant_count's tile loop on keys with runs of tens of thousands; the one pair with taumax == 1
    is the first of the triangle, so q_cor == q_raw only if the divisor is the maximum of ALL pairs"""
    d = _closed_form_pairs(hip_ctx, "cens64-2049", ("global",))
    cls, n_class = _five_classes(d.S)
    counts = _timed("S=2049 censored quantiles, the reference's counts", lambda: dt.group_counts(d, cls))
    assert counts[0][0].max() > 10 * 1024 and d.max_taumax() == 1.0 == d.taumax(0, 1)
    assert d.max_taumax(columns=np.arange(1, d.S)) < 1.0
    bn = (np.nonzero(counts[0][0])[0] - d.K)[1:-1:3]
    got = _timed("S=2049 censored quantiles", lambda: hip_ctx.quantiles(d.X, PROBS, d.value(bn), cls, n_class))
    _assert_quantiles(got, d, cls, PROBS, bn, counts)
