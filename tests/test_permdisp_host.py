"""ici_kendalltau_permdisp without a device: designed raw matrices go to the brute-force checker
(tests/permdisp_checker.py) and, through an engine whose `permdisp` is api._permdisp_numpy on that raw matrix, to the
front end.  What is pinned: the table's integers, the square-root recipe against 120-digit decimals, the identity with
betadisper's principal coordinates, the exact F on points whose answer is known in closed form, the residual
permutation against a loop that permutes the residual vector itself, the degenerate cases and the labellings shared
with the two other tests."""
import math
import os
import random
import re
import warnings
from fractions import Fraction

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests import permdisp_checker as pc
from tests.numpy_ctx import NumpyCtx
from tests.oracle_engine import OracleEngine
from tests.permdisp_checker import bits, na_real

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["statistic", "pvalue", "df_among", "df_within", "ss_among", "ss_within", "n_permutations", "n_ge",
        "n_undefined", "perm_statistic", "distances", "class_mean_distance", "class_size", "class_levels",
        "centroid_distance", "nearest_centroid", "n_negative", "n_valid", "n_na", "sums", "sample_id", "max_taumax",
        "run_time"]
FLOATS = ("statistic", "pvalue", "ss_among", "ss_within", "perm_statistic", "distances", "class_mean_distance",
          "centroid_distance")


class RawEngine(NumpyCtx):
    """the numpy engine with the one method this entry looks for: the integers of a designed raw matrix"""

    def __init__(self, raw):
        self.raw = np.asarray(raw, dtype=np.float64)

    def permdisp(self, X, cls, n_class, global_na=None, perspective="global", alternative="two.sided", continuity=False,
                 flags=0):
        assert X.shape[1] == self.raw.shape[0]
        n_pairs, Q, T = api._permdisp_numpy(self.raw, cls, n_class)
        return n_pairs, Q, T, 0.5, np.zeros(5, dtype=np.int64)


def _front(raw, codes, **kw):
    S = len(codes)
    kw.setdefault("permutations", 19)
    kw.setdefault("seed", 5)
    return api.ici_kendalltau_permdisp(np.zeros((4, S)), list(codes), colnames=[f"s{i}" for i in range(S)],
                                       engine=RawEngine(raw), **kw)


def _both(raw, codes, n_perm=19, seed=5, strata=None):
    codes = np.asarray(codes, dtype=np.int32)
    n_class = int(codes.max()) + 1
    assert len(np.unique(codes)) == n_class            # the levels of the front end are the codes
    got = _front(raw, codes, permutations=n_perm, seed=seed, strata=strata)
    ref = pc.brute_permdisp(raw, codes, n_class, pc.documented_permutations(codes, n_perm, seed, strata))
    assert list(got) == KEYS
    assert got["sums"]["q_total"] == ref["q_total"] and got["sums"]["t"].tolist() == ref["t"]
    assert list(got["sums"]["class_q"]) == ref["class_q"]
    assert (got["n_valid"], got["n_na"]) == tuple(ref["n_pairs"])
    assert (got["df_among"], got["df_within"], got["n_ge"], got["n_undefined"], got["n_negative"]) == \
        (ref["df_among"], ref["df_within"], ref["n_ge"], ref["n_undefined"], ref["n_negative"])
    assert np.array_equal(got["nearest_centroid"], ref["nearest_centroid"])
    assert np.array_equal(got["class_size"], ref["class_size"])
    for key in FLOATS:
        assert np.shape(got[key]) == np.shape(ref[key]) and np.array_equal(bits(got[key]), bits(ref[key])), key
    return got, ref


def _line_raw(x):
    x = np.asarray(x, dtype=np.float64)
    raw = 1.0 - np.abs(x[:, None] - x[None, :])
    assert raw.min() >= -1.0
    return raw


def _random_raw(S, seed, nan=0):
    rng = np.random.default_rng(seed)
    raw = rng.uniform(-1.0, 1.0, (S, S))
    raw = np.triu(raw, 1) + np.triu(raw, 1).T
    np.fill_diagonal(raw, 1.0)
    for _ in range(nan):
        i, j = rng.choice(S, 2, replace=False)
        raw[i, j] = raw[j, i] = np.nan
    return raw


def test_abi_names_and_sources():
    header = open(os.path.join(ROOT, "include", "icikt.h")).read()
    for nm in ("icikt_permdisp_f64", "icikt_permdisp_in", "icikt_permdisp_csc"):
        assert nm in _lib.EXPORTS and re.search(r"\bint " + nm + r"\(", header), nm
    for f in ("icikt_permdisp.hip", "icikt_capi_permdisp.cpp"):
        assert os.path.join(ROOT, "icikendalltau_amd", "csrc", f) in _lib.SOURCES
    assert all(os.path.exists(p) for p in _lib.SOURCES + _lib.HEADERS)
    assert "#define ICIKT_PERMDISP_MAX_CELLS (1ll << 26)" in header and _lib.PERMDISP_MAX_CELLS == 1 << 26
    import icikendalltau_amd
    assert icikendalltau_amd.ici_kendalltau_permdisp is api.ici_kendalltau_permdisp


def test_limbs_combine_to_python_ints_on_both_paths():
    lo = np.array([[0, 1, (1 << 48) - 1], [5, 1 << 32, 7]], dtype=np.int64)
    small = np.array([[0, 3, (1 << 30) - 1], [0, 0, 1]], dtype=np.int64)
    large = np.array([[0, 3, (1 << 36) - 1], [1 << 30, 0, 1]], dtype=np.int64)
    for hi in (small, large):
        T = _lib._limbs_to_ints(lo, hi)
        assert T.dtype == object and T.shape == lo.shape and all(isinstance(v, int) for v in T.ravel())
        assert T.tolist() == [[int(h) * 2 ** 32 + int(l) for l, h in zip(rl, rh)] for rl, rh in zip(lo, hi)]
    assert _lib._limbs_to_ints(lo[:0], small[:0]).shape == (0, 3)


@pytest.mark.parametrize("nan", [0, 5])
def test_the_numpy_integers_are_the_checkers(nan):
    S = 23
    raw = _random_raw(S, 3, nan)
    cls = np.random.default_rng(4).integers(0, 4, S)
    n_pairs, Q, T = api._permdisp_numpy(raw, cls, 6)
    n_val, n_na, Q_ref, T_ref, _A, _sizes = pc.brute_table(raw, cls, 6)
    assert list(n_pairs) == [n_val, n_na] and n_na == nan and Q == Q_ref and isinstance(Q, int)
    assert T.dtype == object and T.tolist() == T_ref and not T[:, 4:].any()


def test_points_on_a_line():
    """dyadic coordinates: every d^2 is exact.  Classes of 4 and 8 points: the centroids are dyadic, z_i is |x_i - mean|
    itself and F the ANOVA of those deviations, in fractions; a class of 3: z_i is the one rounding of |x_i - mean|"""
    rng = np.random.default_rng(8)
    x = rng.integers(0, 2048, 15) / 1024.0                              # multiples of 2^-10 in [0, 2)
    codes = np.array([0] * 4 + [1] * 8 + [2] * 3, dtype=np.int32)
    raw = _line_raw(x)
    got, ref = _both(raw, codes)
    assert got["n_negative"] == 0 and got["n_na"] == 0
    fx = [Fraction(v) for v in x]
    mean = {c: sum(fx[i] for i in range(15) if codes[i] == c) / int((codes == c).sum()) for c in range(3)}
    dev = [abs(fx[i] - mean[codes[i]]) for i in range(15)]
    for i in range(15):
        assert got["distances"][i] == float(dev[i])                     # (Fraction -> float rounds once, correctly)
        if codes[i] < 2:
            assert Fraction(float(got["distances"][i])) == dev[i]       # exactly representable
        for c in range(3):
            assert got["centroid_distance"][i, c] == float(abs(fx[i] - mean[c]))
    assert list(got["nearest_centroid"]) == [min(range(3), key=lambda c: (abs(fx[i] - mean[c]), c)) for i in range(15)]
    # two classes whose deviations are exact: F is the ANOVA of |x_i - mean|, to the bit
    keep = np.flatnonzero(codes < 2)
    got2, _ref2 = _both(raw[np.ix_(keep, keep)], codes[keep])
    F, ss_a, ss_w, df_a, df_w = pc.anova([dev[i] for i in keep], list(codes[keep]), 2)
    assert got2["statistic"] == float(F) and got2["ss_among"] == float(ss_a) and got2["ss_within"] == float(ss_w)
    assert (got2["df_among"], got2["df_within"]) == (df_a, df_w) == (1, 10)
    stat = api.permdisp_statistic(got2["distances"], codes[keep], 2)
    assert stat.F == F and stat.ss_among == ss_a and stat.ss_within == ss_w


def test_a_triple_that_breaks_the_triangle_inequality():
    """class 0: d = 1/4, 1/4, 1 -- the two far points are closer to the third than they may be.  Its centroid lies at a
    negative squared distance from sample 0: X = 3 (1/16 + 1/16) - (1/16 + 1/16 + 1) = -3/4"""
    d = np.ones((6, 6))
    np.fill_diagonal(d, 0.0)
    d[0, 1] = d[1, 0] = d[0, 2] = d[2, 0] = 0.25
    for a, b, v in ((3, 4, 0.5), (3, 5, 0.5), (4, 5, 0.5)):
        d[a, b] = d[b, a] = v
    got, ref = _both(1.0 - d, [0, 0, 0, 1, 1, 1])
    assert got["n_negative"] == 1 and ref["x"][0][0] == -3 * (1 << 50) // 4
    assert got["distances"][0] == math.sqrt(0.75) / 3                    # sqrt(abs(.)), as vegan takes it
    assert got["distances"][3] == float(pc.distance((3 * 2 - 3) * (1 << 48), 3))


def test_the_rounding_recipe_on_its_lattice():
    rng = random.Random(2006)
    cases = [(1, 65535), (1, 1), (0, 7), (2 ** 84 - 1, 65535), (2 ** 84 - 1, 1)]
    for _ in range(20000):
        n = rng.choice((1, 2, 3, 255, 65535, rng.randint(1, 65535)))
        kind = rng.randrange(4)
        X = (rng.randint(0, 999), rng.randint(1, 2 ** 42 - 1) ** 2, rng.getrandbits(rng.randint(1, 84)),
             (rng.randint(1, 2 ** 20) * n) ** 2)[kind]
        cases.append((X, n))
    for X, n in cases:
        assert api.permdisp_distance(X, n) == pc.distance(X, n), (X, n)
        assert api.permdisp_distance(-X, n) == api.permdisp_distance(X, n)
    assert api.permdisp_distance(1, 65535) == 2.0 ** -25 / 65535 >= 2.0 ** -41
    with pytest.raises(ValueError):
        api.permdisp_distance(5, 0)


@pytest.mark.parametrize("S,seed", [(7, 1), (24, 2), (40, 3)])
def test_the_betadisper_identity(S, seed):
    """Gower's principal coordinates with numpy.linalg.eigh: B = -1/2 J d^2 J, the squared distance to a centroid over
    the positive axes minus the negative ones.  eigh's backward error is about S eps ||B||_2 <= 40 x 2.2e-16 x 80 =
    7e-13; the bound on z^2 is 1e-10 absolute, two orders over that (z^2, not z: the root amplifies error near 0)."""
    raw = _random_raw(S, seed)
    assert len(np.unique(raw[np.triu_indices(S, 1)])) == S * (S - 1) // 2
    codes = np.random.default_rng(seed).integers(0, 3, S).astype(np.int32)
    codes[:3] = [0, 1, 2]
    got, ref = _both(raw, codes, n_perm=3)
    d2 = (1.0 - raw) ** 2
    np.fill_diagonal(d2, 0.0)
    J = np.eye(S) - np.ones((S, S)) / S
    lam, V = np.linalg.eigh(-0.5 * J @ d2 @ J)
    Y = V * np.sqrt(np.abs(lam))[None, :]
    sign = np.where(lam > 0, 1.0, -1.0)
    for c in range(3):
        centre = Y[codes == c].mean(axis=0)
        pcoa = ((Y - centre[None, :]) ** 2 * sign[None, :]).sum(axis=1)
        n_c = int((codes == c).sum())
        exact = np.array([float(Fraction(ref["x"][i][c], n_c * n_c << 50)) for i in range(S)])
        z2 = got["centroid_distance"][:, c] ** 2
        print(S, c, "max |D2 - pcoa|", np.abs(exact - pcoa).max(), "max |z^2 - |pcoa||", np.abs(z2 - np.abs(pcoa)).max())
        assert np.abs(exact - pcoa).max() <= 1e-10 and np.abs(z2 - np.abs(pcoa)).max() <= 1e-10


@pytest.mark.parametrize("strata", [None, "two"])
def test_permuting_the_residual_vector_itself(strata):
    S = 24
    raw = _random_raw(S, 9)
    codes = np.array([0] * 6 + [1] * 10 + [2] * 8, dtype=np.int32)
    np.random.default_rng(1).shuffle(codes)
    st = None if strata is None else ["l"] * 11 + ["r"] * 13
    got, ref = _both(raw, codes, n_perm=25, seed=13, strata=st)
    resid = got["distances"] - got["class_mean_distance"][codes]
    assert list(resid) == ref["residuals"]
    labs = api.anosim_permutations(codes, 25, 13, st)
    own = np.argsort(codes, kind="stable")
    Fs = []
    for lab in labs:
        sigma = np.empty(S, dtype=np.int64)
        sigma[own] = np.argsort(lab, kind="stable")       # position i takes the residual of a sample labelled codes[i]
        assert np.array_equal(lab[sigma], codes)
        Fs.append(pc.anova([float(v) for v in resid[sigma]], list(codes), 3)[0])
    assert np.array_equal(bits(got["perm_statistic"]), bits([pc.to_double(f) for f in Fs]))
    obs = ref["exact"][0][0]
    assert got["n_ge"] == sum(1 for f in Fs if f is not None and f >= obs)
    assert got["pvalue"] == float(Fraction(1 + got["n_ge"], 26))


def test_degenerate_cases():
    na = bits(na_real())[0]
    raw = _random_raw(8, 12)
    one, _ = _both(raw, [0] * 8)                                        # one class: distances, no F
    assert bits(one["statistic"])[0] == na and bits(one["pvalue"])[0] == na and one["n_undefined"] == 19
    assert (one["df_among"], one["df_within"]) == (0, 7) and np.all(one["distances"] > 0)
    single, _ = _both(raw, list(range(8)))                              # all singletons: every sample is its centroid
    assert not single["distances"].any() and bits(single["statistic"])[0] == na and single["df_within"] == 0
    assert list(single["nearest_centroid"]) == list(range(8))
    same, _ = _both(np.ones((8, 8)), [0, 0, 0, 1, 1, 1, 2, 2])          # identical columns: raw = 1, all z equal
    assert not same["distances"].any() and bits(same["statistic"])[0] == na and same["sums"]["q_total"] == 0
    assert list(same["nearest_centroid"]) == [0] * 8                    # ties go to the earlier class
    two, _ = _both(raw[:2, :2], [0, 1])                                 # S <= C'
    assert bits(two["statistic"])[0] == na and (two["df_among"], two["df_within"]) == (1, 0)
    # SS_W = 0 < SS_A: two tight classes of different spread
    d = np.array([[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, .5], [1, 1, .5, 0]])
    inf, _ = _both(1.0 - d, [0, 0, 1, 1])
    assert inf["statistic"] == math.inf and list(inf["distances"]) == [0.5, 0.5, 0.25, 0.25]
    assert inf["n_ge"] == sum(1 for v in inf["perm_statistic"] if v == math.inf)


def test_every_value_na_warns_once_and_gives_na():
    raw = np.full((6, 6), np.nan)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got, _ref = _both(raw, [0, 0, 0, 1, 1, 1])
    w = [x for x in w if "PERMDISP" in str(x.message)]
    assert len(w) == 2 - 1 and w[0].category is RuntimeWarning          # (once per front-end call; _both makes one)
    text = str(w[0].message)
    assert "15" in text and "ici_kendalltau_medians" in text and "n_valid" in text
    na = bits(na_real())[0]
    for key in FLOATS:
        assert np.all(bits(got[key]) == na), key
    assert (got["n_valid"], got["n_na"], got["n_ge"], got["n_undefined"], got["n_negative"]) == (0, 15, 0, 19, 0)
    assert (got["df_among"], got["df_within"]) == (1, 4) and np.all(got["nearest_centroid"] == -1)
    assert not got["sums"]["t"].any() and got["sums"]["t"].shape == (6, 2)
    # one NA pair among values: the table is as summed
    raw = _random_raw(6, 2, nan=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        part, _ref = _both(raw, [0, 0, 0, 1, 1, 1])
    assert part["n_na"] == 1 and part["sums"]["t"].any() and np.all(bits(part["distances"]) == na)


def test_the_same_seed_gives_permanovas_labellings():
    S = 12
    raw = _random_raw(S, 6)
    codes = np.array([0, 1, 2] * 4, dtype=np.int32)
    st = ["a"] * 5 + ["b"] * 7
    seen = {}

    class Recorder(RawEngine):
        def permanova(self, X, cls, n_class, perm_cls, *a, **k):
            seen["perms"] = np.array(perm_cls)
            n_pairs, Q, class_q = api._permanova_numpy(self.raw, cls, n_class, perm_cls)
            return n_pairs, Q, class_q, 0.5, np.zeros(5, dtype=np.int64)

    names = [f"s{i}" for i in range(S)]
    api.ici_kendalltau_permanova(np.zeros((4, S)), list(codes), permutations=21, seed=3, strata=st, colnames=names,
                                 engine=Recorder(raw))
    want = api.anosim_permutations(codes, 21, 3, st)
    assert np.array_equal(seen["perms"], want)
    got = _front(raw, codes, permutations=21, seed=3, strata=st)
    ref = pc.brute_permdisp(raw, codes, 3, want)
    assert np.array_equal(bits(got["perm_statistic"]), bits(ref["perm_statistic"])) and got["n_ge"] == ref["n_ge"]
    given = _front(raw, codes, permutations=want, seed=99)              # an array of codes is used as given
    assert np.array_equal(bits(given["perm_statistic"]), bits(got["perm_statistic"]))
    other = np.array([[0] * 11 + [1], [0, 1] * 6, [0] * 12], dtype=np.int64)   # other class sizes; one class: no F
    res = _front(raw, codes, permutations=other)
    ref = pc.brute_permdisp(raw, codes, 3, other)
    assert np.array_equal(bits(res["perm_statistic"]), bits(ref["perm_statistic"])) and res["n_undefined"] == 1


def test_types_and_argument_checks():
    raw = _random_raw(9, 4)
    codes = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    res = _front(raw, codes)
    for key in ("statistic", "pvalue", "ss_among", "ss_within", "max_taumax", "run_time"):
        assert isinstance(res[key], float), key
    for key in ("df_among", "df_within", "n_permutations", "n_ge", "n_undefined", "n_negative", "n_valid", "n_na"):
        assert isinstance(res[key], int) and not isinstance(res[key], bool), key
    assert res["distances"].shape == (9,) and res["centroid_distance"].shape == (9, 3)
    assert res["class_size"].dtype == np.int64 and res["nearest_centroid"].dtype == np.int32
    assert res["sums"]["t"].dtype == object and isinstance(res["sums"]["q_total"], int)
    short = _front(raw, codes, return_perms=False)
    assert list(short) == [k for k in KEYS if k != "perm_statistic"]
    with pytest.raises(ValueError, match="`sample_classes` must give one class per column"):
        api.ici_kendalltau_permdisp(np.zeros((4, 9)), None, colnames=[f"s{i}" for i in range(9)], engine=RawEngine(raw))
    with pytest.raises(ValueError, match="class code outside 0 .. n_class - 1"):
        _front(raw, codes, permutations=np.full((2, 9), 3, dtype=np.int32))
    with pytest.raises(ValueError, match="`permutations` must be in 0"):
        _front(raw, codes, permutations=-1)
    with pytest.raises(ValueError, match="`labels` must give one class per value"):
        api.permdisp_statistic([1.0, 2.0], [0], 1)


def test_an_engine_without_the_method_goes_through_the_full_matrix():
    assert not hasattr(OracleEngine(), "permdisp")
    rng = np.random.default_rng(17)
    X = np.asfortranarray(rng.standard_normal((30, 9)))
    names = [f"s{i}" for i in range(9)]
    codes = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], dtype=np.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = api.ici_kendalltau_permdisp(X, list(codes), permutations=9, seed=2, colnames=names, engine=OracleEngine())
        full = api.ici_kendalltau(X, colnames=names, engine=OracleEngine())
    ref = pc.brute_permdisp(np.asarray(full["raw"]), codes, 3, pc.documented_permutations(codes, 9, 2))
    assert list(got) == KEYS and got["sums"]["t"].tolist() == ref["t"]
    for key in FLOATS:
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
