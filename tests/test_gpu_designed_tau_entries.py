"""The eight later selection entries (padjust, mst, hclust, anosim, cross, the prepared reference with its class table,
permanova, permdisp) on designed matrices whose ICI-Kendall-tau is known in closed form from integers (tests/designed_tau.py).
Their own test files feed a brute-force checker with Context.matrix or Context.cross of the same input: the library is
its own source of values there, on Gaussian columns whose tau clusters round 0.  Here the reference needs no S x S matrix
from the library, so it reaches the key space (raw = -1 and +1, runs of thousands of equal keys), the accumulator bounds
and the sizes (S = 2 049 ... 5 795, the triangle cut in two by the driver) that those files cannot.

Every test first asserts that Context.pairs gives the closed form BITWISE on the first 2 000 combn pairs of its input
(_closed_form_pairs).  From there integers compare as integers and doubles by their bits.  The p-value has no closed
form: a p-value plane is compared with Context.pairs on the same pairs, and padjust's sorted p-values are one
Context.pairs p-value per distinct numerator, repeated by its count.  hclust's reference is
tests/hclust_checker.brute_hclust on the closed-form matrix, which is independent of the library.  The censored family
(test_censored_*, at the end) adds taumax, completeness and max_taumax below 1 and perspectives that differ."""
import numpy as np
import pytest

from icikendalltau_amd import _lib
from tests import designed_tau as dt
from tests import test_gpu_designed_tau as base
from tests.anosim_checker import documented_permutations
from tests.cross_checker import rect_pairs
from tests.hclust_checker import brute_hclust
from tests.mst_checker import brute_mst
from tests.padjust_checker import ALPHAS, METHODS, outputs_from_sorted
from tests.test_gpu_designed_tau import CONFIGS, NA, ONE, _classes, _closed_form_pairs, _no_plan_override, _pvalues, _timed, bits
from tests.test_gpu_medians import _five_classes

pytestmark = pytest.mark.gpu

KEYS130 = ["two-valued", "two-valued-half", "swaps40", "reversals41", "reversals41-wide"]
PERSPECTIVES = ("global", "local")
MEDIAN_STAGE_MAX = 4096         # icikt_medians.hip: the keys of a cell that stage in LDS
PMV_ROW_RUN = 1024              # icikt_permanova.hip: the rows of one workgroup's run in k_pmv_perm
PMV_LDS_CLASSES = 2048          # the classes whose bins k_pmv_classes keeps in LDS
_REF = {}


def _plus_minus(S, n, seed, split=None):
    """every column +-base, no NA column: seeded signs, or + for the columns below `split` and - from there"""
    if split is None:
        signs = np.where(np.random.default_rng(seed).random(S) < 0.4, -1, 1)
    else:
        signs = np.where(np.arange(S) < split, 1, -1)
    return dt.swaps(S, n, seed=seed, params=np.zeros(S, dtype=np.int64), signs=signs)


_MORE = {
    "rev24-520": lambda: dt.reversals(520, 24, seed=3),
    "rev24-2051": lambda: dt.reversals(2051, 24, seed=3),
    "rev24-4100": lambda: dt.reversals(4100, 24, seed=8),
    "rev24-5795": lambda: dt.reversals(5795, 24, seed=5),
    # three prefix lengths (the whole column reversed is the base with the other sign) and two signs: four values of
    # raw, each shared by a thousand or more of a query's partners
    "rev24-4104": lambda: dt.reversals(4104, 24, seed=6, values=[0, 9, 24], flip=0.3),
    "halves-2049": lambda: _plus_minus(2049, 24, 7, split=1024),
    "plus-minus-5794": lambda: _plus_minus(5794, 24, 9),
    # tied, left-censored columns; no two alike but columns 0 and 1, the one pair with taumax == 1.  No column is
    # reflected: every raw is positive (0.96 .. 1), and the largest 15 % of the values connect every sample
    "cens64-5795": lambda: dt.censored(5795, 64, 8, 3, 5, seed=5, n_lib=56, flip=0.0),
}


def _design(key):
    """the designs of tests/test_gpu_designed_tau.py, this file's own, and "<key>/valid": a design's valid columns alone"""
    if key not in base._DESIGN:
        if key in _MORE:
            base._DESIGN[key] = _MORE[key]()
        elif key.endswith("/valid"):
            base._DESIGN[key] = dt.valid_columns(base._design(key[:-len("/valid")]))
    return base._design(key)


def _checked(ctx, key, perspectives=PERSPECTIVES):
    _design(key)
    return _closed_form_pairs(ctx, key, perspectives)


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _layout(d, key, classes):
    """the class layouts of tests/test_gpu_designed_tau.py; on a "/valid" design the same classes of the columns kept"""
    if key.endswith("/valid"):
        full = _design(key[:-len("/valid")])
        cls, n_class = _classes(full, classes)
        return np.ascontiguousarray(cls[full.kind == dt.VALID]), n_class
    return _classes(d, classes)


def _classes_of_two(S, n_class, seed=12):
    """a seeded permutation of repeat(arange(n_class), 2); where 2 n_class < S the samples left over go one each to
    the first classes (S = 4 098 with 2 048 classes: two classes of three)"""
    assert 0 <= S - 2 * n_class <= n_class
    labels = np.concatenate([np.repeat(np.arange(n_class), 2), np.arange(S - 2 * n_class)])
    return np.random.default_rng(seed).permutation(labels).astype(np.int32)


THREE_OF_2049 = (0, 1000, 2048)


def _three_labels(S, layout):
    """the labels of 2 049 declared classes of which three have samples: "sorted" into three blocks, or interleaved"""
    used = np.array(THREE_OF_2049, dtype=np.int32)
    assert S % 3 == 0
    return np.repeat(used, S // 3) if layout == "sorted" else np.ascontiguousarray(used[np.arange(S) % 3])


# ---- anosim and permanova --------------------------------------------------------------------------------------------

def _assert_anosim(got, ref, d):
    n_pairs, w2, nw, n_ge, n_undef, class_w2, class_nw, mx, rc5 = got
    print("M, n_na", n_pairs.tolist(), ref["n_pairs"].tolist(), "labellings", len(w2), "differing w2", int(np.sum(w2 != ref["w2"])),
          "nw", int(np.sum(nw != ref["nw"])), "n_ge", n_ge, ref["n_ge"], "n_undefined", n_undef, ref["n_undefined"])
    assert np.array_equal(n_pairs, ref["n_pairs"])
    assert np.array_equal(w2, ref["w2"]) and np.array_equal(nw, ref["nw"])
    assert n_ge == ref["n_ge"] and n_undef == ref["n_undefined"]
    assert np.array_equal(class_w2, ref["class_w2"]) and np.array_equal(class_nw, ref["class_nw"])
    assert mx == d.max_taumax() and np.array_equal(rc5, d.reason_counts())


def _assert_permanova(got, ref, d):
    n_pairs, Q, class_q, mx, rc5 = got
    want = np.array(ref["class_q"], dtype=object).reshape(class_q.shape)
    print("values, n_na", n_pairs.tolist(), ref["n_pairs"].tolist(), "Q", Q, ref["q_total"], "cells", class_q.size,
          "non-zero", int(np.count_nonzero(want)), "differing cells", int(np.sum(class_q != want)))
    assert np.array_equal(n_pairs, ref["n_pairs"])
    assert isinstance(Q, int) and Q == ref["q_total"]
    assert class_q.tolist() == ref["class_q"]
    assert mx == d.max_taumax() and np.array_equal(rc5, d.reason_counts())


def _small_labels(d, key, classes):
    cls, n_class = _layout(d, key, classes)
    return cls, n_class, documented_permutations(cls, 33, seed=13)


@pytest.mark.parametrize("classes", ["interleaved", "na-class"])
@pytest.mark.parametrize("key", KEYS130)
def test_anosim(hip_ctx, key, classes):
    d = _checked(hip_ctx, key)
    cls, n_class, perms = _small_labels(d, key, classes)
    ref = _ref(("anosim", key, classes), lambda: dt.anosim(d, cls, n_class, perms))
    cnt = dt.group_counts(d)[0][0]
    if key.startswith("two-valued"):      # two runs of thousands of equal keys, at the two ends of the key space
        assert np.count_nonzero(cnt) == 2 and cnt[0] >= 3000 and cnt[2 * d.m] >= 3000
    assert ref["n_pairs"][1] > 0 and ref["n_undefined"] == 0 and 0 < ref["nw"][0] < ref["n_pairs"][0]
    for perspective in PERSPECTIVES:
        _assert_anosim(hip_ctx.anosim(d.X, cls, n_class, perms, None, perspective), ref, d)
    _assert_anosim(hip_ctx.anosim(d.X, cls, n_class, None), dt.anosim(d, cls, n_class, perms[:0]), d)


@pytest.mark.parametrize("key", ["two-valued", "reversals41-wide"])
def test_anosim_under_another_plan(plan_ctx, key):
    d = _checked(plan_ctx, key, ("global",))
    cls, n_class, perms = _small_labels(d, key, "interleaved")
    ref = _ref(("anosim", key, "interleaved"), lambda: dt.anosim(d, cls, n_class, perms))
    plan_ctx.debug_set_plan("anostrip=64,anoperms=3,tkblock=1")
    _assert_anosim(plan_ctx.anosim(d.X, cls, n_class, perms), ref, d)


@pytest.mark.parametrize("key", [k + v for k in KEYS130 for v in ("/valid", "")])
def test_permanova(hip_ctx, key):
    """"/valid": no NA pair, so every class is summed; the whole design has NA columns: Q alone, every A_c zero"""
    d = _checked(hip_ctx, key)
    for classes in (("interleaved",) if key.endswith("/valid") else ("interleaved", "na-class")):
        cls, n_class, perms = _small_labels(d, key, classes)
        ref = _ref(("permanova", key, classes), lambda: dt.permanova(d, cls, n_class, perms))
        if key.endswith("/valid"):
            assert ref["n_pairs"][1] == 0 and sum(ref["class_q"][0]) > 0 and ref["n_undefined"] == 0
            if key.startswith("two-valued"):     # only q = 0 and q = 2^52 are summed
                table = dt.q_table(d)
                assert table[0] == 1 << 52 and table[2 * d.m] == 0 and ref["q_total"] % (1 << 52) == 0
                assert all(a % (1 << 52) == 0 for row in ref["class_q"] for a in row)
        else:
            assert ref["n_pairs"][1] > 0 and not any(any(row) for row in ref["class_q"]) and ref["q_total"] > 0
        for perspective in PERSPECTIVES:
            _assert_permanova(hip_ctx.permanova(d.X, cls, n_class, perms, None, perspective), ref, d)


@pytest.mark.parametrize("key", ["two-valued/valid", "reversals41-wide/valid"])
def test_permanova_under_another_plan(plan_ctx, key):
    d = _checked(plan_ctx, key, ("global",))
    cls, n_class, perms = _small_labels(d, key, "interleaved")
    ref = _ref(("permanova", key, "interleaved"), lambda: dt.permanova(d, cls, n_class, perms))
    plan_ctx.debug_set_plan("anostrip=64,anoperms=3,tkblock=1")
    _assert_permanova(plan_ctx.permanova(d.X, cls, n_class, perms), ref, d)


# ---- permdisp --------------------------------------------------------------------------------------------------------

def _assert_permdisp(got, ref, d, key=None):
    """Context.permdisp's five items against dt.permdisp_table's tuple: the two tables are object arrays of Python ints
    and are compared in one call.  key: the design's, to count its reasons once for all the tests that use it."""
    n_pairs, Q, T, mx, rc5 = got
    n_val, n_na, Q_ref, T_ref, _A, _sizes = ref
    same = T == T_ref if T.shape == T_ref.shape else np.zeros(1, dtype=bool)
    print("values, n_na", n_pairs.tolist(), [n_val, n_na], "Q", Q, Q_ref, "cells", T.size, "non-zero", int(np.count_nonzero(T_ref)),
          "differing cells", int(same.size - np.count_nonzero(same)))
    assert n_pairs.dtype == np.int64 and n_pairs.tolist() == [n_val, n_na]
    assert isinstance(Q, int) and Q == Q_ref
    assert T.dtype == object and T_ref.dtype == object and set(map(type, T.ravel())) <= {int}
    assert T.shape == T_ref.shape and same.dtype == bool and same.all()
    want_rc5 = d.reason_counts() if key is None else _ref(("reason_counts", key), d.reason_counts)
    assert mx == d.max_taumax() and np.array_equal(rc5, want_rc5)


def _na_rows_are_zero(d, ref, got):
    """with NA columns: their rows of the table are all zero -- the all-missing column's and the constant one's --, every
    other row is as summed, and n_na is the pairs that an NA column is part of"""
    k = int(np.sum(d.kind != dt.VALID))
    good = d.kind == dt.VALID
    assert k > 0 and (d.kind == dt.ALL_MISSING).any()
    assert ref[1] == d.S * (d.S - 1) // 2 - (d.S - k) * (d.S - k - 1) // 2 == got[0][1]
    for T in (ref[3], got[2]):
        assert not T[~good].any() and all(row.any() for row in T[good])
    assert ref[2] > 0


@pytest.mark.parametrize("classes", ["interleaved", "na-class"])
@pytest.mark.parametrize("key", [k + v for k in KEYS130 for v in ("/valid", "")])
def test_permdisp(hip_ctx, key, classes):
    """"/valid": no NA pair; the whole design has NA columns, and the table is as summed all the same (PERMANOVA's class
    sums are zero there)"""
    d = _checked(hip_ctx, key)
    cls, n_class = _layout(d, key, classes)
    ref = _ref(("permdisp", key, classes), lambda: dt.permdisp_table(d, cls, n_class))
    assert ref[5][2] == (0 if key.endswith("/valid") or classes == "interleaved" else int(np.sum(d.kind != dt.VALID)))
    assert not ref[3][:, [c for c in range(n_class) if ref[5][c] == 0]].any()          # an empty class: 0 for every sample
    if key.startswith("two-valued"):          # only q = 0 and q = 2^52 are summed: every cell counts its raw = -1 partners
        table = dt.q_table(d)
        assert table[0] == 1 << 52 and table[2 * d.m] == 0 and all(v % (1 << 52) == 0 for v in ref[3].ravel())
        assert max(ref[3].ravel()) >= 20 << 52
    for perspective in PERSPECTIVES:
        got = hip_ctx.permdisp(d.X, cls, n_class, None, perspective)
        _assert_permdisp(got, ref, d)
        if key.endswith("/valid"):
            assert ref[1] == 0 and got[0][1] == 0 and all(row.any() for row in got[2])
        else:
            _na_rows_are_zero(d, ref, got)


@pytest.mark.parametrize("spec", ["tkblock=1", "tkblock=1000"])
@pytest.mark.parametrize("key", ["two-valued", "reversals41-wide/valid"])
def test_permdisp_under_another_plan(plan_ctx, key, spec):
    """tkblock=1: the kept plane is written by one block of the triangle per row"""
    d = _checked(plan_ctx, key, ("global",))
    cls, n_class = _layout(d, key, "interleaved")
    ref = _ref(("permdisp", key, "interleaved"), lambda: dt.permdisp_table(d, cls, n_class))
    plan_ctx.debug_set_plan(spec)
    _assert_permdisp(plan_ctx.permdisp(d.X, cls, n_class), ref, d)


def _front_end(d, cls, n_perm=33, seed=13):
    """api.ici_kendalltau_permdisp on the design with the labels "c<class>", its warnings, and the codes the front end
    gives those labels: the classes that have a sample, renumbered in order"""
    import warnings
    from icikendalltau_amd import api
    levels, codes = np.unique(cls, return_inverse=True)
    assert len(levels) <= 10                               # (the labels sort as the classes do)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = api.ici_kendalltau_permdisp(d.X, ["c%d" % c for c in cls], permutations=n_perm, seed=seed,
                                          colnames=["s%d" % i for i in range(d.S)])
    assert got["class_levels"] == ["c%d" % c for c in levels] and got["n_permutations"] == n_perm
    return got, [str(x.message) for x in w], codes.astype(np.int32), len(levels)


def _assert_front_end(got, ref, d):
    from tests.test_gpu_permdisp import _assert_front
    _assert_front(got, (None, d.max_taumax(), None), ref)


@pytest.mark.parametrize("key", [k + "/valid" for k in KEYS130])
def test_permdisp_front_end(hip_ctx, key):
    """no NA pair: the statistic is defined (the checker's F on the five designs: 94.94, 51.18, 31.61, 15.14, 16.995)"""
    d = _checked(hip_ctx, key, ("global",))
    cls, _n = _layout(d, key, "interleaved")
    got, warned, codes, n_class = _front_end(d, cls)
    ref = _ref(("permdisp front", key), lambda: dt.permdisp(d, codes, n_class, documented_permutations(codes, 33, 13)))
    print(key, "F", ref["statistic"], "p", ref["pvalue"], "n_ge", ref["n_ge"], "n_negative", ref["n_negative"])
    assert ref["n_pairs"][1] == 0 and ref["exact"][0][0] is not None and np.isfinite(ref["statistic"]) and ref["statistic"] > 10
    assert ref["n_undefined"] == 0 and (ref["df_among"], ref["df_within"]) == (4, d.S - 5)
    assert not any("PERMDISP needs every pair" in m for m in warned)
    _assert_front_end(got, ref, d)


def test_permdisp_front_end_with_na_columns(hip_ctx):
    key = "reversals41"
    d = _checked(hip_ctx, key, ("global",))
    cls, _n = _layout(d, key, "interleaved")
    got, warned, codes, n_class = _front_end(d, cls)
    ref = dt.permdisp(d, codes, n_class, documented_permutations(codes, 33, 13))
    assert ref["n_pairs"][1] > 0 and sum(1 for m in warned if "PERMDISP needs every pair" in m) == 1
    _assert_front_end(got, ref, d)
    from tests.test_gpu_permdisp import FLOATS
    for name in FLOATS:
        assert np.all(bits(got[name]) == NA), name
    assert np.all(got["nearest_centroid"] == -1) and got["n_undefined"] == 33 and got["n_ge"] == 0 and got["n_negative"] == 0
    assert got["sums"]["t"].any() and not got["sums"]["t"][d.kind != dt.VALID].any()    # the table is as summed


def test_permdisp_front_end_when_every_own_class_distance_is_zero(hip_ctx):
    """two-valued-half/valid with the column's sign as its class: every raw inside a class is +1, q = 0, so every sample
    sits on its own class's centroid; F is NA ("all values equal") for the observed labelling and every permutation"""
    key = "two-valued-half/valid"
    d = _checked(hip_ctx, key, ("global",))
    cls = (d.sign < 0).astype(np.int32)
    assert dt.is_two_valued(d) and 0 < cls.sum() < d.S
    got, warned, codes, n_class = _front_end(d, cls)
    assert n_class == 2 and np.array_equal(codes, cls) and not any("PERMDISP needs every pair" in m for m in warned)
    ref = dt.permdisp(d, codes, n_class, documented_permutations(codes, 33, 13))
    assert ref["n_pairs"][1] == 0 and ref["class_q"] == [0, 0] and all(row[c] == 0 for row, c in zip(ref["t"], cls))
    assert np.all(bits(ref["distances"]) == 0) and ref["exact"][0][0] is None and bits(ref["statistic"])[0] == NA
    assert ref["n_undefined"] == 33 and ref["n_negative"] == 0 and ref["n_ge"] == 0
    assert all(row[1 - c] == ref["class_size"][1 - c] << 52 for row, c in zip(ref["t"], cls))   # raw = -1 with the other class
    _assert_front_end(got, ref, d)
    assert got["n_undefined"] == got["n_permutations"] == 33 and got["n_negative"] == 0
    assert np.all(bits(got["distances"]) == 0) and bits(got["statistic"])[0] == NA


# ---- padjust ---------------------------------------------------------------------------------------------------------

def _sorted_p(ctx, d, perspective, alternative):
    """one Context.pairs p-value per distinct numerator (|num| for "two.sided"), repeated by its count"""
    one_sided = alternative != "two.sided"
    keys, count, fi, fj, _n_na = dt.pvalue_keys(d, one_sided)
    out, _cnt, _rsn = ctx.pairs(d.X, fi, fj, perspective=perspective, alternative=alternative, want_counts=False)
    p, n_na = dt.sorted_pvalues(d, out[:, 1], one_sided)
    return p, n_na, count


def _assert_padjust(got, ref, d, max_table):
    n_tests, n_rej, cutoff, table, n_table, mx, rc5 = got
    t = min(ref["n_table"], max_table)
    print("n_tests", n_tests.tolist(), "n_rejected", n_rej.tolist(), ref["n_rejected"].tolist(), "n_table", n_table,
          ref["n_table"], "differing", int(np.sum(bits(cutoff) != bits(ref["p_cutoff"]))),
          int(np.sum(bits(table[0]) != bits(ref["table_p"][:t]))) if table.shape[1] == t else "shape")
    assert np.array_equal(n_tests, ref["n_tests"]) and np.array_equal(n_rej, ref["n_rejected"])
    assert np.array_equal(bits(cutoff), bits(ref["p_cutoff"]))
    assert n_table == ref["n_table"] and table.shape == (2, t)
    assert np.array_equal(bits(table[0]), bits(ref["table_p"][:t]))
    assert np.array_equal(bits(table[1]), bits(ref["table_adjusted"][:t]))
    assert mx == d.max_taumax() and np.array_equal(rc5, d.reason_counts())


def _padjust_case(ctx, d, p, n_na, method, perspective, alternative, label=None, short_table=False):
    """the five ALPHAS and, where a run of equal p has more than one unscanned product, a level inside the longest one;
    returns how each level's cut meets the runs"""
    a_in = dt.alpha_inside_a_run(p, method)
    alphas = ALPHAS + (() if a_in is None else (a_in,))
    ref = outputs_from_sorted(p, n_na, method, alphas)
    kinds = dt.cuts_in_runs(p, method, alphas)
    if a_in is not None:
        assert kinds[-1] == "inside"
    rooms = (ref["n_table"], ref["n_table"] + 5) + ((ref["n_table"] // 2,) if short_table else ())
    for room in rooms:
        call = lambda: ctx.padjust(d.X, method, alphas, room, None, perspective, alternative)   # noqa: E731
        got = call() if label is None else _timed(label, call)
        _assert_padjust(got, ref, d, room)
    return kinds


@pytest.mark.parametrize("alternative", ["two.sided", "greater"])
@pytest.mark.parametrize("key", KEYS130)
def test_padjust(hip_ctx, key, alternative):
    d = _checked(hip_ctx, key)
    kinds = set()
    for perspective in PERSPECTIVES:
        p, n_na, count = _sorted_p(hip_ctx, d, perspective, alternative)
        assert count.max() >= 100 and len(p) + n_na == d.S * (d.S - 1) // 2      # hundreds of pairs share a p
        for method in METHODS:
            kinds |= set(_padjust_case(hip_ctx, d, p, n_na, method, perspective, alternative, short_table=True))
    print(key, alternative, "cuts", kinds)
    assert "inside" in kinds                               # the scan alone decided where a whole run of equal p falls
    if alternative == "greater" or key == "reversals41-wide":
        assert "edge" in kinds                             # and a cut where two runs meet, 0 < n_rejected < m


# ---- mst -------------------------------------------------------------------------------------------------------------

def _assert_mst(ctx, got, ref, d, perspective="global", pvalues=True):
    ri, rj, rcomp, rn = ref
    ti, tj, vals, component, n_comp, n_rounds, mx, rc5 = got
    print("S", d.S, "n_tree", len(ti), len(ri), "n_components", n_comp, rn, "n_rounds", n_rounds,
          "differing edges", int(np.sum((ti != ri) | (tj != rj))) if len(ti) == len(ri) else "length")
    assert len(ti) + n_comp == d.S and np.array_equal(ti, ri) and np.array_equal(tj, rj)
    assert np.array_equal(component, rcomp) and n_comp == rn
    raw = d.value(d.num[ri, rj])
    assert vals.shape == (5, len(ri))
    assert np.array_equal(bits(vals[1]), bits(raw)) and np.array_equal(bits(vals[0]), bits(raw))
    assert np.all(bits(vals[3:5]) == ONE)
    if pvalues and len(ri):
        assert np.array_equal(bits(vals[2]), bits(_pvalues(ctx, d, ri, rj, perspective)))
    assert mx == d.max_taumax() and np.array_equal(rc5, d.reason_counts())


def _value_that_hundreds_equal(d, key):
    """the largest numerator that 200 pairs equal; on reversals41-wide, whose hundreds of distinct values are shared by
    fewer pairs each, its most frequent one"""
    cnt = dt.group_counts(d)[0][0]
    floor = 30 if key == "reversals41-wide" else 200
    t = int(np.max(np.nonzero(cnt >= floor)[0])) - d.m
    print(key, "bound", t, "/", d.m, "pairs equal to it", int(cnt[t + d.m]))
    assert cnt[t + d.m] >= (30 if key == "reversals41-wide" else 200)
    return t


@pytest.mark.parametrize("key", KEYS130)
def test_mst(hip_ctx, key):
    d = _checked(hip_ctx, key)
    ref = _ref(("mst", key), lambda: brute_mst(d.raw))
    if key.startswith("two-valued"):
        closed = dt.mst_two_valued(d)
        assert dt.is_two_valued(d) and all(np.array_equal(a, b) for a, b in zip(closed, ref))
        assert int(np.sum(d.num[ref[0], ref[1]] < 0)) == 1            # one bridge of raw = -1 between the sign groups
    t = _value_that_hundreds_equal(d, key)
    bound = _ref(("mst", key, t), lambda: brute_mst(d.raw, float(d.value(t))))
    above = brute_mst(d.raw, float(d.value(t + 1)))
    print(key, "min_raw", t, "/", d.m, "components without a bound, on the value, above it", ref[3], bound[3], above[3])
    assert ref[3] <= bound[3] <= above[3]
    for perspective, scale_max in CONFIGS:
        _assert_mst(hip_ctx, hip_ctx.mst(d.X, None, None, perspective, "two.sided", False, 0, scale_max), ref, d, perspective)
        _assert_mst(hip_ctx, hip_ctx.mst(d.X, float(d.value(t)), None, perspective, "two.sided", False, 0, scale_max), bound,
                    d, perspective)


# ---- hclust ----------------------------------------------------------------------------------------------------------

def _assert_hclust(got, ref, d):
    ra, rb, rsize, rraw, rcomp, rn = ref
    ma, mb, msize, mraw, mcor, component, n_comp, mx, rc5 = got
    same_len = len(ma) == len(ra)
    print("S", d.S, "n_merges", len(ma), len(ra), "n_components", n_comp, rn,
          "differing merges", int(np.sum((ma != ra) | (mb != rb))) if same_len else "length",
          "differing heights", int(np.sum(bits(mraw) != bits(rraw))) if same_len else "length")
    assert len(ma) + n_comp == d.S
    assert np.array_equal(ma, ra) and np.array_equal(mb, rb) and np.array_equal(msize, rsize)
    assert np.array_equal(bits(mraw), bits(rraw)) and np.array_equal(bits(mcor), bits(rraw))     # taumax == 1
    assert np.array_equal(component, rcomp) and n_comp == rn
    assert mx == d.max_taumax() and np.array_equal(rc5, d.reason_counts())


@pytest.mark.parametrize("method", ["complete", "average", "single"])
@pytest.mark.parametrize("key", KEYS130)
def test_hclust(hip_ctx, key, method):
    d = _checked(hip_ctx, key)
    ref = _ref(("hclust", key, method), lambda: brute_hclust(d.raw, method))
    t = _value_that_hundreds_equal(d, key)
    bound = brute_hclust(d.raw, method, float(d.value(t)))
    print(key, method, "min_raw", t, "/", d.m, "merges", len(ref[0]), len(bound[0]))
    assert len(ref[0]) > 100 and 0 < len(bound[0]) <= len(ref[0])
    for perspective, scale_max in CONFIGS:
        _assert_hclust(hip_ctx.hclust(d.X, method, None, None, perspective, "two.sided", False, 0, scale_max), ref, d)
    _assert_hclust(hip_ctx.hclust(d.X, method, float(d.value(t))), bound, d)


# ---- cross and the prepared reference ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref_ctx():
    """the prepared reference's context: every other call on a context drops its reference"""
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def _assert_rect(ctx, got, r, k, perspective, planes=True):
    """Context.cross' six items against the rectangle's integers"""
    out5, idx, vals, n_valid, mx, rc5 = got
    d, Sq, Sr = r.d, r.Sq, r.Sr
    pi, pj = rect_pairs(Sq, Sr)
    pairs, rsn = _ref(("rectangle's pairs", id(d), Sq, perspective),
                      lambda: ctx.pairs(d.X, pi, pj, perspective=perspective, want_counts=False)[::2])
    assert np.array_equal(rsn.reshape(Sq, Sr), r.reasons)
    pv = pairs.reshape(Sq, Sr, 4)
    if planes:
        ok = r.valid
        assert out5.shape == (5, Sq, Sr) and np.all(np.isnan(out5[:, ~ok]))
        want = d.value(r.num)
        assert np.array_equal(bits(out5[1][ok]), bits(want[ok])) and np.array_equal(bits(out5[0][ok]), bits(want[ok]))
        assert np.all(bits(out5[3][ok]) == ONE) and np.all(bits(out5[4][ok]) == ONE)
        assert np.array_equal(bits(out5[2][ok]), bits(np.ascontiguousarray(pv[:, :, 1])[ok]))
    if k is not None:
        ridx, _nums, rraw, rn = dt.cross_topk(d, Sq, k)
        print("Sq", Sq, "Sr", Sr, "k", k, "differing partners", int(np.sum(idx != ridx)))
        assert np.array_equal(n_valid, rn) and np.array_equal(idx, ridx)
        assert np.array_equal(bits(vals[1]), bits(rraw)) and np.array_equal(bits(vals[0]), bits(rraw))
        sel = ridx >= 0
        assert np.all(bits(vals[3:5])[:, sel] == ONE) and np.all(bits(vals)[:, ~sel] == NA)
        rows = np.repeat(np.arange(Sq), k).reshape(Sq, k)
        assert np.array_equal(bits(vals[2][sel]), bits(np.ascontiguousarray(pv[:, :, 1])[rows[sel], ridx[sel]]))
    assert mx == r.max_taumax() and np.array_equal(rc5, r.reason_counts())


def _assert_class_table(got, cm):
    med2, n_valid = got[6], got[7]
    print("cells", n_valid.size, "differing", int(np.sum(bits(med2[1]) != bits(cm["med"]))))
    assert np.array_equal(n_valid, cm["n_valid"])
    assert np.array_equal(bits(med2[1]), bits(cm["med"])) and np.array_equal(bits(med2[0]), bits(cm["med"]))


def _ref_classes(d, Sq):
    """the reference columns' classes of the interleaved layout with the NA columns moved into class 2 -- a class of NA
    columns alone -- and one more class index that no column has: an empty class"""
    cls, n_class = _classes(d, "na-class")
    return np.ascontiguousarray(cls[Sq:]), n_class + 1


@pytest.mark.parametrize("Sq", [5, 8])
@pytest.mark.parametrize("key", ["two-valued", "swaps40", "reversals41", "reversals41-wide"])
def test_cross_and_cross_prepared(hip_ctx, ref_ctx, key, Sq):
    d = _checked(hip_ctx, key)
    r = dt.rect(d, Sq)
    ref_cls, n_class = _ref_classes(d, Sq)
    cm = dt.cross_class_table(d, Sq, ref_cls, n_class)
    sizes = np.bincount(ref_cls, minlength=n_class)
    assert sizes[2] > 0 and np.all(d.kind[Sq:][ref_cls == 2] != dt.VALID) and sizes[-1] == 0
    assert np.all(cm["n_valid"][:, [2, -1]] == 0) and np.all(bits(cm["med"][:, [2, -1]]) == NA)
    even = (cm["n_valid"] > 0) & (cm["n_valid"] % 2 == 0)
    print(key, Sq, "even cells: edge of a run", int((even & (cm["k_in"] + 1 == cm["run"])).sum()), "inside",
          int((even & (cm["k_in"] + 1 < cm["run"])).sum()))
    _idx, nums, _raw, n_valid = dt.cross_topk(d, Sq, 7)
    tied = (n_valid == 7) & ((r.valid & (r.num >= nums[:, 6][:, None])).sum(axis=1) > 7)
    print(key, Sq, "queries with more than k candidates equal to or above the k-th", int(tied.sum()))
    if key != "reversals41-wide":
        assert tied.any()                                     # the reference index alone decides the k-th place
    ref_ctx.prepare_reference(r.R, 8)
    for perspective, scale_max in CONFIGS:
        for k in (1, 7, r.Sr):
            got = hip_ctx.cross(r.Q, r.R, k, k == 7, None, perspective, "two.sided", False, 0, scale_max)
            _assert_rect(hip_ctx, got, r, k, perspective, planes=k == 7)
            prepared = ref_ctx.cross_prepared(r.Q, k, k == 7, ref_cls, n_class, perspective, "two.sided", False, 0, scale_max)
            _assert_rect(hip_ctx, prepared[:6], r, k, perspective, planes=k == 7)
            _assert_class_table(prepared, cm)


# ---- at the sizes where the kernels change behaviour (the natural plan) ------------------------------------------------

def test_2049_samples_anosim(hip_ctx, monkeypatch):
    """2 098 176 pairs: more than 2 048 x 1 024; nine strips of 256 columns and eight runs of 256 rows of k_anosim_perm"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-2049", ("global",))
    assert d.S * (d.S - 1) // 2 > 2048 * 1024
    cls, n_class = _five_classes(d.S)
    perms = documented_permutations(cls, 33, seed=13)
    ref = _timed("S=2049 anosim, the reference", lambda: dt.anosim(d, cls, n_class, perms))
    _assert_anosim(_timed("S=2049 anosim", lambda: hip_ctx.anosim(d.X, cls, n_class, perms)), ref, d)


def test_2051_samples_anosim_and_permanova(hip_ctx, monkeypatch):
    """No NA column, so PERMANOVA sums every class; S - 1 = 2 050 rows above the last column: three runs of
    k_pmv_perm's 1 024 rows meet in the column sums (S = 2 049 has exactly two), nine runs of k_anosim_perm's 256"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-2051", ("global",))
    assert d.S * (d.S - 1) // 2 > 2048 * 1024 and d.S - 1 > PMV_ROW_RUN * 2 and d.S - 1 > 256 * 8
    cls, n_class = _five_classes(d.S)
    perms = documented_permutations(cls, 33, seed=13)
    ref = _timed("S=2051 permanova, the reference", lambda: dt.permanova(d, cls, n_class, perms))
    assert ref["n_pairs"][1] == 0 and all(all(row) for row in ref["class_q"])
    _assert_permanova(_timed("S=2051 permanova", lambda: hip_ctx.permanova(d.X, cls, n_class, perms)), ref, d)
    ref = _timed("S=2051 anosim, the reference", lambda: dt.anosim(d, cls, n_class, perms))
    _assert_anosim(_timed("S=2051 anosim", lambda: hip_ctx.anosim(d.X, cls, n_class, perms)), ref, d)


def test_2049_samples_permanova_with_na_columns(hip_ctx, monkeypatch):
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-2049", ("global",))
    cls, n_class = _five_classes(d.S)
    perms = documented_permutations(cls, 5, seed=13)
    ref = dt.permanova(d, cls, n_class, perms)
    assert ref["n_pairs"][1] == 2 * d.S - 3 and ref["q_total"] > 0 and not any(any(row) for row in ref["class_q"])
    _assert_permanova(_timed("S=2049 permanova, NA columns", lambda: hip_ctx.permanova(d.X, cls, n_class, perms)), ref, d)


def test_2049_samples_permanova_at_the_accumulator_bound(hip_ctx, monkeypatch):
    """Columns 0 ... 1 023 are +base, the others -base.  For a column j >= 1 024 the first run of k_pmv_perm's rows is
    1 024 values of raw = -1, q = 2^52 each: acc = 2^62, the bound written at the top of icikt_permanova.hip, and Q is
    1 024 x 1 025 x 2^52, about 2^72, across both limbs.  One class; then two classes, class 0 the columns below 1 536,
    which still holds the whole first run of 512 columns, with five other labellings."""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "halves-2049", ("global",))
    table = dt.q_table(d)
    q_of = table[(d.num[:PMV_ROW_RUN, :] + d.m)]                           # the first run of every column
    assert table[0] == 1 << 52 and table[2 * d.m] == 0
    one = np.zeros(d.S, dtype=np.int32)
    two = (np.arange(d.S) >= 1536).astype(np.int32)
    for cls, n_class, n_perm in ((one, 1, 0), (two, 2, 5)):
        acc = [int(q_of[cls[:PMV_ROW_RUN] == cls[j], j].sum()) for j in (PMV_ROW_RUN, 1535, d.S - 1)]
        print("classes", n_class, "acc of the first run of columns 1024, 1535, 2048:", acc)
        assert acc[0] == acc[1] == 1 << 62                                    # acc = 2^62 reached
        perms = documented_permutations(cls, n_perm, seed=13)
        ref = dt.permanova(d, cls, n_class, perms)
        assert ref["q_total"] == 1024 * 1025 * (1 << 52) and ref["n_pairs"].tolist() == [d.S * (d.S - 1) // 2, 0]
        assert ref["class_q"][0] == ([ref["q_total"]] if n_class == 1 else [1024 * 512 * (1 << 52), 0])
        got = _timed("S=2049 permanova at acc = 2^62, %d class(es)" % n_class,
                     lambda: hip_ctx.permanova(d.X, cls, n_class, perms if n_perm else None))
        _assert_permanova(got, ref, d)


def test_4098_samples_permanova_bins_in_global_memory(hip_ctx, monkeypatch):
    """2 049 classes of two samples: more than the 2 048 classes whose bins fit in LDS, so k_pmv_classes adds to its
    bins in global memory, and every bin of the observed labelling holds the q of its one pair"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-4098", ("global",))
    n_class = d.S // 2
    assert n_class > PMV_LDS_CLASSES and (d.kind == dt.VALID).all()
    cls = np.random.default_rng(12).permutation(np.repeat(np.arange(n_class), 2)).astype(np.int32)
    perms = documented_permutations(cls, 3, seed=13)
    ref = _timed("S=4098 permanova, the reference", lambda: dt.permanova(d, cls, n_class, perms))
    table = dt.q_table(d)
    first = np.array([np.nonzero(cls == c)[0] for c in range(n_class)])
    assert ref["class_q"][0] == [int(table[d.num[a, b] + d.m]) for a, b in first]
    print("non-zero bins of the observed labelling", sum(1 for a in ref["class_q"][0] if a), "of", n_class)
    assert sum(1 for a in ref["class_q"][0] if a) > 0.9 * n_class
    _assert_permanova(_timed("S=4098 permanova, 2049 classes", lambda: hip_ctx.permanova(d.X, cls, n_class, perms)), ref, d)


def test_2049_samples_padjust(hip_ctx, monkeypatch):
    """2 098 176 pairs: chip-wide scans over about 2 000 chunks of 1 024 keys, runs of equal p tens of thousands long"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-2049", ("global",))
    assert d.S * (d.S - 1) // 2 > 2048 * 1024
    p, n_na, count = _sorted_p(hip_ctx, d, "global", "two.sided")
    assert count.max() > 10 * 1024
    kinds = set()
    for method in METHODS:
        kinds |= set(_padjust_case(hip_ctx, d, p, n_na, method, "global", "two.sided", "S=2049 padjust " + method))
    print("cuts", kinds)
    assert "inside" in kinds


def test_2049_samples_mst(hip_ctx, monkeypatch):
    """Boruvka rounds over 2 098 176 pairs with a few hundred distinct keys: the combn index decides nearly every edge"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-2049", ("global",))
    assert d.S * (d.S - 1) // 2 > 2048 * 1024
    ref = _timed("S=2049 mst, the reference", lambda: brute_mst(d.raw))
    assert len(np.unique(d.num[d.valid])) < 600 and ref[3] == 3
    _assert_mst(hip_ctx, _timed("S=2049 mst", lambda: hip_ctx.mst(d.X)), ref, d)


@pytest.mark.parametrize("method", ["complete", "average", "single"])
def test_520_samples_hclust(hip_ctx, monkeypatch, method):
    """ceil(520 / 256) = 3 merge workgroups, the last with a tail of 8 slots.  tests/test_designed_tau_host.py shows
    that an average update with one product fused into the sum changes the merge order on this design."""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-520", ("global",))
    assert d.S > 2 * 256 and d.S % 256 != 0
    ref = _timed("S=520 hclust %s, the reference" % method, lambda: brute_hclust(d.raw, method))
    assert len(ref[0]) == d.S - 1
    _assert_hclust(_timed("S=520 hclust " + method, lambda: hip_ctx.hclust(d.X, method)), ref, d)


def test_4099_reference_columns_cross(hip_ctx, ref_ctx, monkeypatch):
    """Sq = 5 against Sr = 4 099.  k = 256: with 24 rows a query has thousands of partners equal to its k-th, so flush
    after flush of k_cross_topk is decided by the reference index.  A class of 4 097 members re-reads its keys past
    MEDIAN_STAGE_MAX, one of 4 096 is the largest that stages; classes of 1 and 2, and an empty class."""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-4104", ("global",))
    Sq, k = 5, 256
    r = dt.rect(d, Sq)
    assert r.Sr == 4099 and r.valid.all()
    _idx, nums, _raw, n_valid = dt.cross_topk(d, Sq, k)
    equal_kth = (r.num == nums[:, k - 1][:, None]).sum(axis=1)
    beyond = (r.num >= nums[:, k - 1][:, None]).sum(axis=1)
    print("partners equal to the k-th", equal_kth.tolist(), "at or above it", beyond.tolist())
    assert np.all(n_valid == k) and np.all(beyond > k) and equal_kth.max() > 1000     # more than k candidates equal to the k-th
    got = _timed("Sq=5 Sr=4099 cross", lambda: hip_ctx.cross(r.Q, r.R, k))
    _assert_rect(hip_ctx, got, r, k, "global")
    ref_ctx.prepare_reference(r.R, Sq)
    order = np.random.default_rng(21).permutation(r.Sr)
    for sizes in ((4097, 1, 0, 1), (4096, 2, 0, 1)):
        ref_cls = np.empty(r.Sr, dtype=np.int32)
        ref_cls[order] = np.repeat(np.arange(4), sizes)
        assert np.bincount(ref_cls, minlength=4).tolist() == list(sizes)
        assert (sizes[0] > MEDIAN_STAGE_MAX) == (sizes[0] == 4097)                    # class size > MEDIAN_STAGE_MAX
        cm = dt.cross_class_table(d, Sq, ref_cls, 4)
        assert cm["n_valid"][0].tolist() == list(sizes) and np.all(bits(cm["med"][:, 2]) == NA)
        got = _timed("Sq=5 Sr=4099 cross_prepared, class of %d" % sizes[0],
                     lambda: ref_ctx.cross_prepared(r.Q, k, True, ref_cls, 4))
        _assert_rect(hip_ctx, got[:6], r, k, "global")
        _assert_class_table(got, cm)


def _cut_in_two(d):
    S = d.S
    total = S * (S - 1) // 2
    assert total > 1 << 24                                # pairs > 2^24 = kTriangleBlockPairs: the driver cuts the triangle
    assert S > 5794 or (S - 1) * (S - 2) // 2 <= 1 << 24  # (5 794 is the smallest S at which it does)
    return total


def test_5794_samples_anosim(hip_ctx, monkeypatch):
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-5794", ("global",))
    _cut_in_two(d)
    cls, n_class = _five_classes(d.S)
    perms = documented_permutations(cls, 4, seed=13)
    ref = _timed("S=5794 anosim, the reference", lambda: dt.anosim(d, cls, n_class, perms))
    _assert_anosim(_timed("S=5794 anosim", lambda: hip_ctx.anosim(d.X, cls, n_class, perms)), ref, d)


@pytest.mark.parametrize("method", ["BH", "holm"])
def test_5794_samples_padjust(hip_ctx, monkeypatch, method):
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-5794", ("global",))
    _cut_in_two(d)
    p, n_na, _count = _ref("sorted p of rev24-5794", lambda: _sorted_p(hip_ctx, d, "global", "two.sided"))
    kinds = _padjust_case(hip_ctx, d, p, n_na, method, "global", "two.sided", "S=5794 padjust " + method)
    assert "inside" in kinds


def test_5794_samples_permanova_with_na_columns(hip_ctx, monkeypatch):
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-5794", ("global",))
    total = _cut_in_two(d)
    cls, n_class = _five_classes(d.S)
    perms = documented_permutations(cls, 2, seed=13)
    ref = _timed("S=5794 permanova, the reference", lambda: dt.permanova(d, cls, n_class, perms))
    assert ref["n_pairs"].sum() == total and ref["n_pairs"][1] == 2 * d.S - 3
    _assert_permanova(_timed("S=5794 permanova, NA columns", lambda: hip_ctx.permanova(d.X, cls, n_class, perms)), ref, d)


def test_5795_samples_permanova(hip_ctx, monkeypatch):
    """no NA column, so the classes are summed across the block cut"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-5795", ("global",))
    _cut_in_two(d)
    cls, n_class = _five_classes(d.S)
    perms = documented_permutations(cls, 4, seed=13)
    ref = _timed("S=5795 permanova, the reference", lambda: dt.permanova(d, cls, n_class, perms))
    assert ref["n_pairs"][1] == 0 and all(all(row) for row in ref["class_q"])
    _assert_permanova(_timed("S=5795 permanova", lambda: hip_ctx.permanova(d.X, cls, n_class, perms)), ref, d)


def test_5795_samples_permdisp(hip_ctx, monkeypatch):
    """no NA column.  The same plane and the same q as PERMANOVA's: n_pairs and Q are its, and A_c = 1/2 sum_{i in c}
    T[i][c] is its class sum of the observed labelling"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-5795", ("global",))
    _cut_in_two(d)
    cls, n_class = _five_classes(d.S)
    ref = _timed("S=5795 permdisp, the reference", lambda: dt.permdisp_table(d, cls, n_class))
    assert ref[1] == 0 and all(ref[4]) and all(row.all() for row in ref[3])
    got = _timed("S=5795 permdisp", lambda: hip_ctx.permdisp(d.X, cls, n_class))
    _assert_permdisp(got, ref, d, "rev24-5795")
    p_pairs, p_Q, p_class_q, _mx, _rc5 = _timed("S=5795 permanova, observed labelling",
                                                lambda: hip_ctx.permanova(d.X, cls, n_class, None))
    assert np.array_equal(got[0], p_pairs) and got[1] == p_Q
    twice = [sum(got[2][cls == c, c]) for c in range(n_class)]
    assert all(v % 2 == 0 for v in twice) and [v // 2 for v in twice] == list(p_class_q[0]) == ref[4]
    base._DESIGN.pop("rev24-5795")
    _REF.pop(("reason_counts", "rev24-5795"), None)


def test_5794_samples_mst(hip_ctx, monkeypatch):
    """every column +-base, no NA column: the closed-form forest -- two stars and one bridge -- across the block cut"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "plus-minus-5794", ("global",))
    _cut_in_two(d)
    assert dt.is_two_valued(d)
    ref = dt.mst_two_valued(d)
    assert ref[3] == 1 and int(np.sum(d.num[ref[0], ref[1]] < 0)) == 1
    _assert_mst(hip_ctx, _timed("S=5794 mst", lambda: hip_ctx.mst(d.X)), ref, d)
    base._DESIGN.pop("plus-minus-5794")


# ---- permdisp at those sizes: k_disp_table's partner loop, its two bin paths, the wave's shortcut and the block cut -------

def _permdisp_at_size(ctx, key, cls, n_class, label, check=None):
    """the reference, `check` on the reference BEFORE the library is called, the call, the comparison"""
    d = _design(key)
    ref = _timed(label + ", the reference", lambda: dt.permdisp_table(d, cls, n_class))
    if check is not None:
        check(ref)
    got = _timed(label, lambda: ctx.permdisp(d.X, cls, n_class))
    _assert_permdisp(got, ref, d, key)
    return got, ref


def test_2049_samples_permdisp_with_na_columns(hip_ctx, monkeypatch):
    """nine trips of k_disp_table's loop over 256 partners, the last with one; an all-missing and a constant column"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-2049", ("global",))
    assert -(-d.S // 256) == 9 and sorted(d.kind[d.kind != dt.VALID].tolist()) == [dt.ALL_MISSING, dt.CONSTANT]
    cls, n_class = _five_classes(d.S)
    got, ref = _permdisp_at_size(hip_ctx, "rev24-2049", cls, n_class, "S=2049 permdisp, NA columns")
    assert ref[1] == 2 * d.S - 3
    _na_rows_are_zero(d, ref, got)


@pytest.mark.parametrize("labels", ["one", "two-sorted", "two-interleaved"])
def test_2049_samples_permdisp_at_the_wave_bound(hip_ctx, monkeypatch, labels):
    """Columns 0 ... 1 023 are +base, the 1 025 others -base: raw = -1 across, q = 2^52, hi limb 2^20 and lo limb 0.
    Class-sorted (one class, or two split at 1 024 = 16 waves) every full wave of partners holds one class and takes the
    shortcut: a wave of 64 partners of the other sign sums hi to 64 x 2^20 = 2^26, the bound of a wave's sum written
    at the top of icikt_permdisp.hip, with equality.  Interleaved, every wave holds both classes and each lane adds its
    own limbs: the same matrix through the other path."""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "halves-2049", ("global",))
    S, cut = d.S, 1024
    table = dt.q_table(d)
    assert table[0] == 1 << 52 and table[2 * d.m] == 0 and np.all(d.num[:cut, cut:] == -d.m)
    assert np.all(d.num[:cut, :cut][~np.eye(cut, dtype=bool)] == d.m)
    assert 64 * (table[0] >> 32) == 1 << 26 and table[0] & 0xFFFFFFFF == 0 and cut % 64 == 0           # a full wave's hi sum
    cls = {"one": np.zeros(S, dtype=np.int32), "two-sorted": (np.arange(S) >= cut).astype(np.int32),
           "two-interleaved": (np.arange(S) % 2).astype(np.int32)}[labels]
    n_class = 1 if labels == "one" else 2

    def check(ref):
        T = ref[3]
        lo, hi = dt.permdisp_limbs(d, cls, n_class)
        assert not lo.any() and ref[1] == 0 and ref[2] == cut * (S - cut) << 52
        if labels == "one":
            assert all(T[i, 0] == (S - cut) << 52 for i in range(cut)) and all(T[i, 0] == cut << 52 for i in range(cut, S))
        elif labels == "two-sorted":        # a + sample's cell of the - class, and the other way round; the own class: 0
            assert all(T[i, 1] == 1025 << 52 and T[i, 0] == 0 for i in range(cut))
            assert all(T[i, 0] == 1024 << 52 and T[i, 1] == 0 for i in range(cut, S))
            assert np.all(hi[:cut, 1] == 1025 << 20) and ref[4] == [0, 0]
        else:                               # per class the partners of the other sign, 512 or 513 of them
            other = np.array([[np.sum(cls[cut:] == c) for c in (0, 1)], [np.sum(cls[:cut] == c) for c in (0, 1)]])
            assert np.array_equal(T, (other[(np.arange(S) >= cut).astype(int)]).astype(object) * (1 << 52))
            assert sorted(other.ravel().tolist()) == [512, 512, 512, 513]

    _permdisp_at_size(hip_ctx, "halves-2049", cls, n_class, "S=2049 permdisp at a wave's 2^26, " + labels, check)


@pytest.mark.parametrize("key,n_class", [("rev24-4098", PMV_LDS_CLASSES), ("rev24-4100", PMV_LDS_CLASSES + 2)])
def test_permdisp_either_side_of_the_classes_that_fit_in_lds(hip_ctx, monkeypatch, key, n_class):
    """Classes of two samples (S = 4 098: two of three).  2 048 classes: the bins fill k_disp_table's 32 KB of LDS;
    2 050: they are the sample's own row of the table in global memory, added to with global atomics.  17 trips of the
    partner loop, and rows of the triangle thousands of pairs apart in the column role."""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, key, ("global",))
    assert (n_class <= PMV_LDS_CLASSES) == (key == "rev24-4098") and (d.kind == dt.VALID).all()
    cls = _classes_of_two(d.S, n_class)
    sizes = np.bincount(cls, minlength=n_class)
    assert sizes.min() == 2 and sizes.max() == (3 if key == "rev24-4098" else 2)

    def check(ref):
        table = dt.q_table(d)
        assert ref[1] == 0 and np.count_nonzero(ref[3]) > 0.9 * ref[3].size
        pairs = [np.nonzero(cls == c)[0] for c in range(n_class) if sizes[c] == 2]
        assert [ref[4][c] for c in range(n_class) if sizes[c] == 2] == [int(table[d.num[a, b] + d.m]) for a, b in pairs]

    _permdisp_at_size(hip_ctx, key, cls, n_class, "S=%d permdisp, %d classes" % (d.S, n_class), check)
    if key == "rev24-4100":
        base._DESIGN.pop(key)
        _REF.pop(("reason_counts", key), None)


@pytest.mark.parametrize("layout", ["sorted", "interleaved"])
def test_4098_samples_permdisp_global_bins_that_accumulate(hip_ctx, monkeypatch, layout):
    """2 049 declared classes, so the bins are in global memory, and three of them used by 1 366 samples each: a cell
    collects up to 1 366 values through global atomics (a class of two samples gets at most two).  Sorted into three
    blocks, the waves of one class add their sums with one atomic per limb; interleaved, every lane adds its own."""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-4098", ("global",))
    n_class = PMV_LDS_CLASSES + 1
    cls = _three_labels(d.S, layout)
    assert np.bincount(cls, minlength=n_class)[list(THREE_OF_2049)].tolist() == [1366] * 3

    def check(ref):
        lo, hi = dt.permdisp_limbs(d, cls, n_class)
        used = lo[:, list(THREE_OF_2049)]
        print("lo-limb sums of the used cells: min", int(used.min()).bit_length(), "max", int(used.max()).bit_length(), "bits")
        assert used.min() >= 1 << 32 and ref[1] == 0                   # every used cell carries out of 32 bits
        assert np.count_nonzero(lo) == np.count_nonzero(hi) == 3 * d.S

    got, _ref_ = _permdisp_at_size(hip_ctx, "rev24-4098", cls, n_class, "S=4098 permdisp, 3 of 2049 classes, " + layout, check)
    assert np.count_nonzero(got[2]) == 3 * d.S and got[2][:, list(THREE_OF_2049)].all()     # an unused class: 0 in every row


def test_5794_samples_permdisp_with_na_columns(hip_ctx, monkeypatch):
    """the kept plane written by two blocks of the triangle; 23 trips of the partner loop; NA columns"""
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "rev24-5794", ("global",))
    total = _cut_in_two(d)
    cls, n_class = _five_classes(d.S)
    got, ref = _permdisp_at_size(hip_ctx, "rev24-5794", cls, n_class, "S=5794 permdisp, NA columns")
    assert ref[0] + ref[1] == total and ref[1] == 2 * d.S - 3
    _na_rows_are_zero(d, ref, got)


# ---- the censored family: taumax, completeness and cor differ from each other, from raw and from 1 ---------------------

CENS130 = ["cens64", "cens64-ties", "cens64-apart"]


def _first_part_holds_the_maximum(d, Sq):
    """the design's columns reordered: query 0 has a partner at the largest taumax of all pairs, the other queries have
    none, and neither has the reference: the rectangle's maximum lies in the first stitched part alone"""
    a, b = np.nonzero(d.valid)
    tm = np.full((d.S, d.S), -np.inf)
    tm[a, b] = d.taumax(a, b)
    row_max = tm.max(axis=1)
    top = row_max.max()
    q0 = int(np.argmax(row_max == top))
    rest = np.nonzero((row_max < top) & (d.kind == dt.VALID))[0][:Sq - 1]
    assert len(rest) == Sq - 1
    queries = np.concatenate([[q0], rest])
    return d.columns(np.concatenate([queries, np.setdiff1d(np.arange(d.S), queries)]))


@pytest.mark.parametrize("spec", ["tkblock=1", "tkblock=4200"])
@pytest.mark.parametrize("key", CENS130)
def test_censored_mst_and_cross(plan_ctx, ref_ctx, key, spec):
    """the tree's five values per edge, and the rectangle with its top-k and class table, scaled by the rectangle's own
    maximum -- below the stacked triangle's on the designs with a twin pair among the queries -- and, from a prepared
    reference with room for 3 of the 8 queries (the front end stitches three parts), rescaled across the parts"""
    ctx = plan_ctx
    d0 = _checked(ctx, key)
    S, Sq, k = d0.S, 8, 7
    ctx.debug_set_plan(spec)
    for perspective, scale_max in CONFIGS:
        d = d0.under(perspective)
        p_of = base._p_of(ctx, d, perspective)
        tail = (None, perspective, "two.sided", False, 0, scale_max)
        mx_all, rc5 = d.max_taumax(), d.reason_counts()
        ref = _ref(("mst", key, perspective), lambda: brute_mst(d.raw))
        ti, tj, vals, component, n_comp, _rounds, mx, grc = ctx.mst(d.X, None, *tail)
        assert np.array_equal(ti, ref[0]) and np.array_equal(tj, ref[1]) and np.array_equal(component, ref[2]) and n_comp == ref[3]
        want = dt.carried(d, ref[0], ref[1], mx_all, scale_max, p_of(ref[0], ref[1]))
        print(key, spec, perspective, scale_max, "mst planes differing", [int(np.sum(bits(vals[q]) != bits(want[q]))) for q in range(5)])
        assert np.array_equal(bits(vals), bits(want)) and mx == mx_all and np.array_equal(grc, rc5)
        # the rectangle
        dd = _first_part_holds_the_maximum(d, Sq) if key == "cens64-apart" else d
        pp = p_of if dd is d else base._p_of(ctx, dd, perspective)
        r = dt.rect(dd, Sq)
        mx_r = r.max_taumax()
        parts = [r.max_taumax(np.arange(q, min(q + 3, Sq))) for q in range(0, Sq, 3)]
        print("max_taumax: triangle", dd.max_taumax(), "rectangle", mx_r, "stitched parts", parts)
        if key == "cens64-apart":
            assert parts[0] == mx_r and max(parts[1:]) < mx_r
        elif perspective == "global":
            assert mx_r < dd.max_taumax() == 1.0                      # both twins are queries
        qa, ra = np.nonzero(r.valid)
        want5 = np.full((5, Sq, r.Sr), np.nan)
        want5[:, qa, ra] = dt.carried(dd, qa, ra + Sq, mx_r, scale_max, pp(qa, ra + Sq))
        idx, _keys, _raw, n_valid = dt.cross_topk(dd, Sq, k)
        qrows = np.arange(Sq)[:, None]
        wantk = dt.carried(dd, qrows, np.where(idx >= 0, idx + Sq, -1), mx_r, scale_max,
                           pp(np.broadcast_to(qrows, idx.shape), np.maximum(idx, 0) + Sq))
        ref_cls, n_class = _ref_classes(dd, Sq)
        cm = dt.cross_class_table(dd, Sq, ref_cls, n_class)
        got = ctx.cross(r.Q, r.R, k, True, *tail)
        ref_ctx.prepare_reference(r.R, Sq)
        prepared = ref_ctx.cross_prepared(r.Q, k, True, ref_cls, n_class, perspective, "two.sided", False, 0, scale_max)
        for out5, gidx, vals, gn, mx, grc in (got, prepared[:6]):
            ok = r.valid
            assert np.all(np.isnan(out5[:, ~ok])) and np.array_equal(bits(out5[:, ok]), bits(want5[:, ok]))
            assert np.array_equal(gidx, idx) and np.array_equal(gn, n_valid) and np.array_equal(bits(vals), bits(wantk))
            assert mx == mx_r and np.array_equal(grc, r.reason_counts())
        med2, gnv = prepared[6], prepared[7]
        assert np.array_equal(gnv, cm["n_valid"]) and np.array_equal(bits(med2[1]), bits(cm["med"]))
        assert np.array_equal(bits(med2[0]), bits(dt.median_cor(dd, cm, mx_r) if scale_max else cm["med"]))
        # the front end against a reference prepared with room for 3 of the 8 queries: three stitched parts
        from icikendalltau_amd import api
        levels = np.unique(ref_cls)
        import warnings
        with warnings.catch_warnings(), api.prepare_reference(r.R, 3, reference_names=["r%d" % i for i in range(r.Sr)],
                                                              reference_classes=["c%d" % c for c in ref_cls]) as kept:
            warnings.simplefilter("ignore")
            res = api.ici_kendalltau_cross(r.Q, kept, k, True, perspective=perspective, scale_max=scale_max,
                                           query_names=["q%d" % i for i in range(Sq)])
        assert res["class_levels"] == ["c%d" % c for c in levels] and len(levels) < 10 and res["max_taumax"] == mx_r
        for f, name in enumerate(("cor", "raw", "pvalue", "taumax", "completeness")):
            got5, gotk = np.asarray(res[name], dtype=np.float64), np.asarray(res["topk_" + name], dtype=np.float64)
            assert np.array_equal(bits(got5[ok]), bits(want5[f][ok])), name
            assert np.array_equal(bits(gotk), bits(wantk[f])), name
        assert np.array_equal(np.asarray(res["indices"]), idx) and np.array_equal(np.asarray(res["class_n_valid"]), cm["n_valid"][:, levels])
        med_cor = (dt.median_cor(dd, cm, mx_r) if scale_max else cm["med"])[:, levels]
        got_raw, got_cor = (np.asarray(res[q], dtype=np.float64) for q in ("class_med_raw", "class_med_cor"))
        print("stitched class table: cells", got_cor.size, "med_cor differing", int(np.sum(bits(got_cor) != bits(med_cor))))
        assert np.array_equal(bits(got_raw), bits(cm["med"][:, levels]))
        assert np.array_equal(bits(got_cor), bits(med_cor))
        # and without the matrix: no part keeps its raw, so a part below the call's maximum is asked for it once more
        with warnings.catch_warnings(record=True) as told, api.prepare_reference(
                r.R, 3, reference_names=["r%d" % i for i in range(r.Sr)], reference_classes=["c%d" % c for c in ref_cls]) as kept:
            warnings.simplefilter("always")
            asked, batch = [], kept._batch
            kept._batch = lambda *a: (asked.append(a[2]), batch(*a))[1]                 # a[2]: want_matrix
            res = api.ici_kendalltau_cross(r.Q, kept, None, False, perspective=perspective, scale_max=scale_max,
                                           query_names=["q%d" % i for i in range(Sq)])
        again = asked[3:]
        told = [str(x.message) for x in told if str(x.message).startswith("Warning:")]
        print("split without the matrix: parts asked again", len(again), "warnings", len(told))
        assert asked[:3] == [False] * 3 and (len(again) == 2 and all(again)) == (key == "cens64-apart" and scale_max)
        assert "raw" not in res and res["max_taumax"] == mx_r
        assert len(told) == r.reason_counts()[2:].sum() > 0       # one per pair with a constant column, asked again or not
        assert np.array_equal(bits(np.asarray(res["class_med_cor"], dtype=np.float64)), bits(med_cor))
        assert np.array_equal(bits(np.asarray(res["class_med_raw"], dtype=np.float64)), bits(cm["med"][:, levels]))


@pytest.mark.parametrize("key", CENS130)
def test_censored_entries_of_raw_alone(hip_ctx, key):
    """anosim, permanova, permdisp, padjust and hclust take raw (or the p-value) alone; on censored columns the two
    perspectives give different matrices, max_taumax is not 1 and raw has ties"""
    d0 = _checked(hip_ctx, key)
    for perspective in PERSPECTIVES:
        d = d0.under(perspective)
        cls, n_class, perms = _small_labels(d, key, "interleaved")
        _assert_anosim(hip_ctx.anosim(d.X, cls, n_class, perms, None, perspective), dt.anosim(d, cls, n_class, perms), d)
        _assert_permanova(hip_ctx.permanova(d.X, cls, n_class, perms, None, perspective), dt.permanova(d, cls, n_class, perms), d)
        _assert_permdisp(hip_ctx.permdisp(d.X, cls, n_class, None, perspective), dt.permdisp_table(d, cls, n_class), d)
        v = dt.valid_columns(d)
        vcls = np.ascontiguousarray(cls[d.kind == dt.VALID])
        vperms = documented_permutations(vcls, 33, seed=13)
        ref = dt.permanova(v, vcls, n_class, vperms)
        assert ref["n_pairs"][1] == 0 and sum(ref["class_q"][0]) > 0
        _assert_permanova(hip_ctx.permanova(v.X, vcls, n_class, vperms, None, perspective), ref, v)
        keys, count, fi, fj, _n_na = dt.pvalue_keys(d)
        p, n_na = dt.sorted_pvalues(d, base._pvalues(hip_ctx, d, fi, fj, perspective))
        for method in ("BH", "holm"):
            _padjust_case(hip_ctx, d, p, n_na, method, perspective, "two.sided")
        for method in ("complete", "average", "single"):
            _assert_hclust_raw(hip_ctx.hclust(d.X, method, None, None, perspective), brute_hclust(d.raw, method), d)


def _assert_hclust_raw(got, ref, d):
    """_assert_hclust where taumax != 1: the heights of cor are those of raw, each divided by max_taumax (the tree is
    built on raw; one more float64 division per height)"""
    ra, rb, rsize, rraw, rcomp, rn = ref
    ma, mb, msize, mraw, mcor, component, n_comp, mx, rc5 = got
    assert np.array_equal(ma, ra) and np.array_equal(mb, rb) and np.array_equal(msize, rsize)
    assert np.array_equal(bits(mraw), bits(rraw)) and np.array_equal(component, rcomp) and n_comp == rn
    assert mx == d.max_taumax() and np.array_equal(rc5, d.reason_counts())
    print("hclust cor heights differing from raw / max_taumax", int(np.sum(bits(mcor) != bits(rraw / mx))), "of", len(rraw))
    assert np.array_equal(bits(mcor), bits(rraw / mx))


# ---- the censored family at the sizes where the kernels change behaviour (the natural plan, global) -------------------

def test_2049_samples_censored_padjust(hip_ctx, monkeypatch):
    _no_plan_override(monkeypatch)
    d = _checked(hip_ctx, "cens64-2049", ("global",))
    p, n_na, count = _sorted_p(hip_ctx, d, "global", "two.sided")
    assert count.max() > 10 * 1024 and len(p) + n_na == d.S * (d.S - 1) // 2
    kinds = _padjust_case(hip_ctx, d, p, n_na, "BH", "global", "two.sided", "S=2049 censored padjust BH")
    assert "inside" in kinds
    base._DESIGN.pop("cens64-2049")


def _censored_cut_in_two(ctx):
    """cens64-5795 with what the four tests below presuppose: the driver cuts the triangle, the largest taumax (1, the
    pair (0, 1)) lies in the first block and every pair of the second block is strictly below it"""
    d = _checked(ctx, "cens64-5795", ("global",))
    S = d.S
    _cut_in_two(d)
    first_rows = int(np.searchsorted(np.cumsum(S - 1 - np.arange(S)), 1 << 24, side="right"))   # whole rows within 2^24 pairs
    later = _ref("cens64-5795 later blocks", lambda: d.max_taumax(columns=np.arange(first_rows, S)))
    mx = _ref("cens64-5795 max", d.max_taumax)
    print("rows of the first block", first_rows, "max_taumax", mx, "of the later rows", later)
    assert 1 < first_rows < S - 2 and d.taumax(0, 1) == mx == 1.0 and later < 1.0
    assert d.max_taumax(columns=np.arange(1, S)) < 1.0                     # no other pair reaches it
    return d


def test_5795_samples_censored_class_matrix(hip_ctx, monkeypatch):
    """med_cor == med_raw (a division by 1.0) only if the divisor comes from the first block"""
    _no_plan_override(monkeypatch)
    d = _censored_cut_in_two(hip_ctx)
    cls, n_class = _five_classes(d.S)
    cm = _timed("S=5795 censored class_matrix, the reference", lambda: dt.class_matrix(d, cls, n_class))
    med2, n_valid, mx, rc5 = _timed("S=5795 censored class_matrix", lambda: hip_ctx.class_matrix(d.X, cls, n_class))
    assert np.array_equal(n_valid, cm["n_valid"]) and np.array_equal(bits(med2[1]), bits(cm["med"]))
    assert np.array_equal(bits(med2[0]), bits(dt.median_cor(d, cm, 1.0))) and mx == 1.0
    assert np.array_equal(rc5, _ref(("reason_counts", "cens64-5795"), d.reason_counts))


def test_5795_samples_censored_anosim(hip_ctx, monkeypatch):
    _no_plan_override(monkeypatch)
    d = _censored_cut_in_two(hip_ctx)
    cls, n_class = _five_classes(d.S)
    perms = documented_permutations(cls, 4, seed=13)
    ref = _timed("S=5795 censored anosim, the reference", lambda: dt.anosim(d, cls, n_class, perms))
    _assert_anosim(_timed("S=5795 censored anosim", lambda: hip_ctx.anosim(d.X, cls, n_class, perms)), ref, d)


def test_5795_samples_censored_permanova(hip_ctx, monkeypatch):
    _no_plan_override(monkeypatch)
    d = _censored_cut_in_two(hip_ctx)
    cls, n_class = _five_classes(d.S)
    perms = documented_permutations(cls, 4, seed=13)
    ref = _timed("S=5795 censored permanova, the reference", lambda: dt.permanova(d, cls, n_class, perms))
    assert ref["n_pairs"][1] == 0 and all(all(row) for row in ref["class_q"])
    _assert_permanova(_timed("S=5795 censored permanova", lambda: hip_ctx.permanova(d.X, cls, n_class, perms)), ref, d)


def test_5795_samples_censored_mst(hip_ctx, monkeypatch):
    """tests/mst_checker.brute_mst as the reference.  It is given the 15 % largest values alone: Kruskal takes the edges
    in the strict order, so when those already connect every sample (asserted) the forest is the unbounded one"""
    _no_plan_override(monkeypatch)
    d = _censored_cut_in_two(hip_ctx)
    cnt = dt.group_counts(d)[0][0]
    above = np.cumsum(cnt[::-1])
    t = d.K - int(np.searchsorted(above, 0.15 * above[-1]))
    ref = _timed("S=5795 censored mst, the reference", lambda: brute_mst(d.raw, float(d.value(t))))
    assert ref[3] == 1 and len(ref[0]) == d.S - 1
    ti, tj, vals, component, n_comp, _rounds, mx, rc5 = _timed("S=5795 censored mst", lambda: hip_ctx.mst(d.X))
    assert np.array_equal(ti, ref[0]) and np.array_equal(tj, ref[1]) and np.array_equal(component, ref[2]) and n_comp == 1
    want = dt.carried(d, ref[0], ref[1], 1.0, True, base._p_of(hip_ctx, d, "global")(ref[0], ref[1]))
    print("mst planes differing", [int(np.sum(bits(vals[q]) != bits(want[q]))) for q in range(5)])
    assert np.array_equal(bits(vals), bits(want)) and mx == 1.0
    base._DESIGN.pop("cens64-5795")
    _REF.pop(("reason_counts", "cens64-5795"), None)
