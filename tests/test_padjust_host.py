"""icikt_padjust's contract without a GPU: the brute-force checker (tests/padjust_checker.py) against scipy's
false_discovery_control and against a direct O(m^2) restatement of the definitions, the consistency of n_rejected with
p_cutoff, api.ici_kendalltau_padjust / ici_kendalltau_significant on an engine without a padjust method (the CPU oracle)
against the checker, the method names, the refusals and the header <-> export agreement for the new symbols."""
import os
import re
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.oracle_engine import OracleEngine
from tests.padjust_checker import (ALPHAS, METHODS, NA_REAL_BITS, adjust_sorted, adjust_sorted_fast, bits, brute_padjust,
                                   outputs_from_sorted)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vectors(n_vec, rng, max_len):
    """sorted p-vectors with ties, zeros and subnormal values"""
    for k in range(n_vec):
        m = int(rng.integers(1, max_len + 1))
        p = rng.random(m)
        kind = k % 5
        if kind == 1:
            p = np.round(p, 1)                                  # long runs of equal values
        elif kind == 2:
            p[rng.random(m) < 0.3] = 0.0
        elif kind == 3:
            p = p * 10.0 ** rng.integers(-320, -300, m)          # subnormal and tiny normal values
        elif kind == 4:
            p = rng.choice(np.array([0.0, 5e-324, 1e-310, 1e-8, 0.03, 0.03, 0.5, 1.0]), m)
        yield np.sort(p)


def test_bh_is_scipys_false_discovery_control_bitwise():
    stats = pytest.importorskip("scipy.stats")
    if not hasattr(stats, "false_discovery_control"):
        pytest.skip("scipy has no false_discovery_control")
    rng = np.random.default_rng(190)
    for p in _vectors(200, rng, 400):
        want = np.sort(stats.false_discovery_control(p, method="bh"))
        assert np.array_equal(bits(adjust_sorted(p, "BH")), bits(want))
        assert np.array_equal(bits(adjust_sorted_fast(p, "BH")), bits(want))


def _direct(p, method):
    """the definitions, O(m^2): every maximum and minimum over its whole index range"""
    m = len(p)
    out = np.empty(m)
    for i in range(m):
        if method == "bonferroni":
            v = float(m) * p[i]
        elif method == "holm":
            v = max(float(m + 1 - (j + 1)) * p[j] for j in range(i + 1))
        else:
            v = min(float(m + 1 - (j + 1)) * p[j] for j in range(i, m))
        out[i] = min(1.0, v)
    return out


@pytest.mark.parametrize("method", ["bonferroni", "holm", "hochberg"])
def test_against_the_definitions(method):
    rng = np.random.default_rng(191)
    for p in _vectors(60, rng, 200):
        want = _direct(p, method)
        assert np.array_equal(bits(adjust_sorted(p, method)), bits(want))
        assert np.array_equal(bits(adjust_sorted_fast(p, method)), bits(want))


@pytest.mark.parametrize("method", METHODS)
def test_sequence_is_monotone_constant_on_runs_and_cutoffs_are_consistent(method):
    rng = np.random.default_rng(192)
    alphas = (0.0, 1e-300, 0.01, 0.05, 0.5, 1.0)
    for p in _vectors(100, rng, 300):
        out = outputs_from_sorted(p, 0, method, alphas, fast=False)
        adj = out["adjusted"]
        assert np.all(np.diff(adj) >= 0)
        same = p[1:] == p[:-1]
        assert np.array_equal(bits(adj[1:][same]), bits(adj[:-1][same]))
        for a, alpha in enumerate(alphas):
            n = out["n_rejected"][a]
            if n == 0:
                assert bits(out["p_cutoff"])[a] == NA_REAL_BITS and not np.any(adj <= alpha)
            else:
                assert np.array_equal(adj <= alpha, p <= out["p_cutoff"][a])
        most = out["n_rejected"].max()
        assert np.array_equal(out["table_p"], np.unique(p[:most]))
        assert out["n_table"] == len(np.unique(p[:most]))
        assert np.array_equal(bits(out["table_adjusted"]), bits(adj[np.searchsorted(p, out["table_p"])]))


@pytest.fixture(scope="module")
def small():
    """60 features x 14 samples with missing cells, a constant column (sample 4: NA with every partner) and a duplicated
    column (p-values tie)"""
    rng = np.random.default_rng(193)
    X = rng.standard_normal((60, 14))
    X[rng.random(X.shape) < 0.1] = np.nan
    X[:, 4] = 2.5
    X[:, 9] = X[:, 2]
    X[:, 11] = 0.5 * X[:, 3] + 0.5 * rng.standard_normal(60)
    names = [f"s{i}" for i in range(14)]
    return X, names


def _full(X, names, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return api.ici_kendalltau(X, colnames=names, engine=OracleEngine(), **kw)


@pytest.mark.parametrize("method", METHODS + ("fdr",))
def test_numpy_path_and_front_end_against_the_checker(small, method):
    X, names = small
    full = _full(X, names)
    name = "BH" if method == "fdr" else method
    ref = brute_padjust(np.asarray(full["pvalue"]), name, ALPHAS, fast=False)
    got = api._padjust_numpy(np.asarray(full["pvalue"]), name, ALPHAS)
    assert np.array_equal(got[0], ref["n_tests"]) and np.array_equal(got[1], ref["n_rejected"])
    assert np.array_equal(bits(got[2]), bits(ref["p_cutoff"]))
    assert np.array_equal(bits(got[3]), bits(ref["table_p"])) and np.array_equal(bits(got[4]), bits(ref["table_adjusted"]))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = api.ici_kendalltau_padjust(X, method=method, alpha=ALPHAS, colnames=names, engine=OracleEngine())
    msgs = [str(x.message) for x in w if str(x.message) in _lib.REASON_WARNINGS.values()]
    assert len(msgs) == 13                                      # the constant column's pairs
    assert res["method"] == name and np.array_equal(res["alpha"], np.asarray(ALPHAS))
    assert res["n_tests"] == ref["n_tests"][0] == 91 - 13 and res["n_na"] == 13
    assert np.array_equal(res["n_rejected"], ref["n_rejected"])
    assert np.array_equal(bits(res["p_cutoff"]), bits(ref["p_cutoff"]))
    assert res["n_table"] == ref["n_table"] == len(res["table_p"])
    assert np.array_equal(bits(res["table_p"]), bits(ref["table_p"]))
    assert np.array_equal(bits(res["table_adjusted"]), bits(ref["table_adjusted"]))
    assert res["n_rejected"][-1] == res["n_tests"] and res["n_rejected"][1] > 0     # alpha = 1 rejects every test
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cut = api.ici_kendalltau_padjust(X, method=method, alpha=1.0, max_table=3, colnames=names, engine=OracleEngine())
    assert cut["n_table"] == ref["n_table"] > 3 and len(cut["table_p"]) == len(cut["table_adjusted"]) == 3
    assert np.array_equal(bits(cut["table_p"]), bits(ref["table_p"][:3])) and cut["alpha"].tolist() == [1.0]


@pytest.mark.parametrize("method", ["BH", "holm"])
def test_significant_against_the_checker(small, method):
    X, names = small
    full = _full(X, names)
    pv, raw = np.asarray(full["pvalue"]), np.asarray(full["raw"])
    ref = brute_padjust(pv, method, (0.05,), fast=False)
    iu, ju = np.triu_indices(len(names), k=1)
    with np.errstate(invalid="ignore"):                         # (NA_real_ is a signalling NaN)
        tri = pv[iu, ju] + 0.0
    lookup = dict(zip(bits(ref["sorted_p"]).tolist(), ref["adjusted"].tolist()))
    tri_adj = np.array([lookup.get(b, np.nan) for b in bits(tri).tolist()])
    with np.errstate(invalid="ignore"):
        keep = tri_adj <= 0.05                                  # the brute-force selection, in combn order
    assert 0 < keep.sum() == ref["n_rejected"][0] < len(tri)
    res = api.ici_kendalltau_significant(X, alpha=0.05, method=method, colnames=names, engine=OracleEngine())
    assert np.array_equal(res["i"], iu[keep]) and np.array_equal(res["j"], ju[keep])
    assert np.array_equal(bits(res["adjusted"]), bits(tri_adj[keep]))
    assert np.array_equal(bits(res["pvalue"]), bits(pv[iu, ju][keep]))
    assert res["n_edges"] == res["n_rejected"] == keep.sum() and res["method"] == method and res["alpha"] == 0.05
    assert bits(np.array([res["p_cutoff"]]))[0] == bits(ref["p_cutoff"])[0]
    # the caller's other bounds cut further; the adjustment stays over all tests
    bound = float(np.median(np.abs(raw[iu, ju][keep])))
    sub = api.ici_kendalltau_significant(X, alpha=0.05, method=method, min_raw=bound, absolute=True, colnames=names,
                                         engine=OracleEngine())
    keep2 = keep & (np.abs(raw[iu, ju]) >= bound)
    assert 0 < keep2.sum() < keep.sum()
    assert np.array_equal(sub["i"], iu[keep2]) and np.array_equal(bits(sub["adjusted"]), bits(tri_adj[keep2]))
    assert sub["n_rejected"] == keep.sum()


def test_significant_without_a_rejection_makes_one_call(small):
    X, names = small
    calls = []

    class Counting(OracleEngine):
        def pairs(self, *args, **kw):
            calls.append("pairs")
            return super().pairs(*args, **kw)

    eng = Counting()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        before = len(calls)
        res = api.ici_kendalltau_significant(X, alpha=0.0, method="bonferroni", colnames=names, engine=eng)
        one = len(calls) - before
        api.ici_kendalltau_significant(X, alpha=0.05, method="bonferroni", colnames=names, engine=eng)
        two = len(calls) - before - one
    assert res["n_edges"] == 0 and res["n_rejected"] == 0 and len(res["i"]) == len(res["adjusted"]) == 0
    assert res["degree"].shape == (14,) and not res["degree"].any() and np.isnan(res["p_cutoff"])
    for key in ("s1", "s2", "cor", "raw", "pvalue", "taumax", "completeness"):
        assert len(res[key]) == 0
    assert one > 0 and two == 2 * one                           # nothing rejected: all pairs once, not twice


def test_method_names_and_refusals(small):
    X, names = small
    eng = OracleEngine()
    assert [api._padjust_method(v) for v in ("bonferroni", "holm", "hochberg", "BH", "fdr")] == \
        ["bonferroni", "holm", "hochberg", "BH", "BH"]
    for bad in ("bh", "Holm", "FDR", "none", "b", "", None, 3):
        with pytest.raises(ValueError, match="bonferroni, holm, hochberg, BH"):
            api.ici_kendalltau_padjust(X, method=bad, colnames=names, engine=eng)
    for bad in ("BY", "hommel"):
        with pytest.raises(ValueError, match=f"{bad}.*not provided"):
            api.ici_kendalltau_padjust(X, method=bad, colnames=names, engine=eng)
    for bad in (np.nan, -0.1, 1.5, (), tuple([0.5] * 17), (0.5, np.nan)):
        with pytest.raises(ValueError, match="`alpha`"):
            api.ici_kendalltau_padjust(X, alpha=bad, colnames=names, engine=eng)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="`max_table`"):
            api.ici_kendalltau_padjust(X, max_table=bad, colnames=names, engine=eng)
    with pytest.raises(ValueError, match="Colnames"):
        api.ici_kendalltau_padjust(X, engine=eng)
    with pytest.raises(ValueError, match="No comparisons to do"):
        api.ici_kendalltau_padjust(X[:, :1], colnames=names[:1], engine=eng)
    for bad in ((0.05, 0.1), np.nan, 2, "0.05", True):
        with pytest.raises(ValueError, match="`alpha` must be one number"):
            api.ici_kendalltau_significant(X, alpha=bad, colnames=names, engine=eng)
    with pytest.raises(ValueError, match="not provided"):
        api.ici_kendalltau_significant(X, method="BY", colnames=names, engine=eng)


def test_engines_pass_their_flags_on():
    seen = []

    class Recorder:
        def padjust(self, *args):
            seen.append(args)
            return "result"

    for cls_ in (api.HipEngine, api.MultiHipEngine):
        eng = object.__new__(cls_)
        eng.ctx = eng._single = Recorder()
        eng.flags = _lib.FLAG_EXACT_INT64
        assert eng.padjust("X", "BH", (0.05,), 7, None, "global", "two.sided", False, _lib.FLAG_TIMING) == "result"
        assert seen[-1] == ("X", "BH", (0.05,), 7, None, "global", "two.sided", False,
                            _lib.FLAG_EXACT_INT64 | _lib.FLAG_TIMING)


def test_exports():
    import icikendalltau_amd as pkg
    assert pkg.ici_kendalltau_padjust is api.ici_kendalltau_padjust
    assert pkg.ici_kendalltau_significant is api.ici_kendalltau_significant
    src = open(os.path.join(ROOT, "include", "icikt.h")).read()
    defs = dict(re.findall(r"#define\s+(ICIKT_[A-Z0-9_]+)\s+\(?(-?\d+)u?\)?", src))
    for name, code in _lib.ADJUST.items():
        assert int(defs["ICIKT_ADJUST_" + name.upper()]) == code
    assert sorted(_lib.ADJUST) == sorted(api.PADJUST_METHODS) and sorted(_lib.ADJUST.values()) == [0, 1, 2, 3]
    assert int(defs["ICIKT_ADJUST_MAX_ALPHA"]) == _lib.ADJUST_MAX_ALPHA == 16
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(icikt_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.EXPORTS)              # what tests/test_abi.py holds the library to
    for nm in ("icikt_padjust_f64", "icikt_padjust_in", "icikt_padjust_csc"):
        assert nm in _lib.EXPORTS
        assert re.search(rf"\bint {nm}\s*\(", src), nm
    for f in ("icikt_padjust.hip", "icikt_capi_padjust.cpp"):
        assert os.path.join(ROOT, "icikendalltau_amd", "csrc", f) in _lib.SOURCES
    assert hasattr(api.HipEngine, "padjust") and hasattr(api.MultiHipEngine, "padjust")
    assert hasattr(_lib.Context, "padjust")
    if not _lib.needs_build():
        import ctypes
        _lib.lib()
        L = ctypes.CDLL(_lib.LIB_PATH)
        for nm in ("icikt_padjust_f64", "icikt_padjust_in", "icikt_padjust_csc"):
            assert hasattr(L, nm), nm
