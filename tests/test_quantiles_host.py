"""api.ici_kendalltau_quantiles on an engine without a quantiles method (the CPU oracle): the reduction from the full
result (api._quantiles_numpy) against the brute-force checker (tests/quantiles_checker.py), the checker itself against
np.sort and np.quantile and on hand-written matrices, the argument errors of the Python layer and the exports."""
import os
import re
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api
from tests.oracle_engine import OracleEngine
from tests.quantiles_checker import NA_REAL_BITS, PROBS, bits, brute_quantiles, group_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nan = float("nan")


def _symmetric(S, seed, na=0.1, ties=False):
    rng = np.random.default_rng(seed)
    raw = rng.uniform(-1, 1, (S, S))
    if ties:
        raw = np.round(raw * 8) / 8          # few distinct values, exact zeros of both signs
        raw[raw == 0.0] *= rng.choice([-1.0, 1.0], raw.shape)[raw == 0.0]
    raw = np.triu(raw, 1)
    raw[np.triu(rng.random((S, S)) < na, 1)] = nan
    raw = raw + raw.T
    np.fill_diagonal(raw, 1.0)
    cor = raw / 0.75
    return [cor, raw, raw, raw, raw]


@pytest.mark.parametrize("ties", [False, True])
def test_checker_against_sort_and_np_quantile(ties):
    S = 40
    out5 = _symmetric(S, 3, ties=ties)
    cls = np.random.default_rng(5).integers(0, 3, S)
    breaks = np.linspace(-1, 1, 12)
    q2, order2, n_valid, n_na, hist, outside = brute_quantiles(out5, cls, PROBS, breaks)
    iu, ju, masks = group_masks(S, cls)
    assert masks[0].sum() == S * (S - 1) // 2 and np.array_equal(masks[1] ^ masks[2], masks[0])
    for g, mask in enumerate(masks):
        x = out5[1][iu, ju][mask]
        assert n_na[g] == np.isnan(x).sum() and n_valid[g] + n_na[g] == mask.sum() and n_valid[g] > 10
        xs = np.sort(x[~np.isnan(x)] + 0.0)
        v = len(xs)
        for k, p in enumerate(PROBS):
            index = 1 + (v - 1) * p
            assert order2[g, k, 0] == xs[int(np.floor(index)) - 1] and order2[g, k, 1] == xs[int(np.ceil(index)) - 1]
            want = np.quantile(xs, p, method="linear")
            assert abs(q2[1, g, k] - want) <= 4 * np.spacing(max(abs(want), 2.0 ** -10)), (g, p)
            wantc = np.quantile(xs / 0.75, p, method="linear")
            assert abs(q2[0, g, k] - wantc) <= 4 * np.spacing(max(abs(wantc), 2.0 ** -10)), (g, p)
            assert not (q2[1, g, k] == 0.0 and np.signbit(q2[1, g, k]))
        assert q2[1, g, 0] == xs[0] and q2[1, g, 1] == xs[-1]                  # p = 0 and p = 1
        assert bits(q2[1, g, 2]) == bits(q2[1, g, 6])                          # the repeated prob
        assert hist[g].sum() + outside[g].sum() == n_valid[g] and outside[g].sum() == 0
    assert np.array_equal(n_valid[1] + n_valid[2], n_valid[0]) and np.array_equal(hist[1] + hist[2], hist[0])
    # the package's own numpy routine states the same contract
    got = api._quantiles_numpy(out5[0], out5[1], cls, PROBS, breaks)
    for a, b in zip(got, (q2, order2, n_valid, n_na, hist, outside)):
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


def test_checker_edge_cases():
    """Four samples, classes {0, 1} and {2, 3}.  Within: pair (0, 1) = 0.5 (v = 1) and the NA pair (2, 3).  Between: -0.0,
    -1.25 (below the breaks), 0.25, 1.0 (the last break itself)."""
    raw = np.zeros((4, 4))
    for (i, j), val in {(0, 1): 0.5, (2, 3): nan, (0, 2): -0.0, (0, 3): -1.25, (1, 2): 0.25, (1, 3): 1.0}.items():
        raw[i, j] = raw[j, i] = val
    out5 = [raw / 2.0, raw, raw, raw, raw]
    cls = np.array([0, 0, 1, 1])
    breaks = np.array([-1.0, 0.0, 0.5, 1.0])
    q2, order2, n_valid, n_na, hist, outside = brute_quantiles(out5, cls, (0.5, 0.0, 1.0, 0.5), breaks)
    assert n_valid.tolist() == [5, 1, 4] and n_na.tolist() == [1, 1, 0]
    assert hist.tolist() == [[0, 2, 2], [0, 0, 1], [0, 2, 1]]       # 0.5 and 1.0 share the closed last bin
    assert outside.tolist() == [[1, 0], [0, 0], [1, 0]]
    assert q2[1, 0].tolist() == [0.25, -1.25, 1.0, 0.25]
    assert q2[1, 1].tolist() == [0.5, 0.5, 0.5, 0.5] and q2[0, 1].tolist() == [0.25] * 4     # v = 1: every prob the value
    # between: -1.25, 0, 0.25, 1: the median interpolates 0 (from -0.0, returned as +0) and 0.25
    assert q2[1, 2].tolist() == [0.125, -1.25, 1.0, 0.125]
    assert order2[2, 0].tolist() == [0.0, 0.25] and not np.signbit(order2[2, 0, 0])
    # v = 0: a group of NA pairs alone, and one above the last break
    raw2 = raw.copy()
    raw2[0, 1] = raw2[1, 0] = nan
    raw2[1, 3] = raw2[3, 1] = 1.5
    q2b, order2b, n_valid_b, n_na_b, hist_b, outside_b = brute_quantiles([raw2, raw2, raw2, raw2, raw2], cls, (0.5,), breaks)
    assert n_valid_b.tolist() == [4, 0, 4] and n_na_b.tolist() == [2, 2, 0]
    assert bits(q2b[:, 1]).tolist() == [[int(NA_REAL_BITS)]] * 2 and np.all(bits(order2b[1]) == NA_REAL_BITS)
    assert hist_b[1].tolist() == [0, 0, 0] and outside_b.tolist() == [[1, 1], [0, 0], [1, 1]]
    # no classes: one group; no probs, no breaks: empty arrays of the right shapes
    q2c, order2c, n_valid_c, n_na_c, hist_c, outside_c = brute_quantiles(out5, None, (), None)
    assert q2c.shape == (2, 1, 0) and order2c.shape == (1, 0, 2) and hist_c.shape == (1, 0)
    assert n_valid_c.tolist() == [5] and n_na_c.tolist() == [1] and outside_c.tolist() == [[0, 0]]
    for r in (raw, raw2):
        got = api._quantiles_numpy(r / 2.0, r, cls, (0.5, 0.0, 1.0, 0.5), breaks)
        ref = brute_quantiles([r / 2.0, r, r, r, r], cls, (0.5, 0.0, 1.0, 0.5), breaks)
        for a, b in zip(got, ref):
            assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


@pytest.fixture(scope="module")
def small():
    """30 features x 12 samples with missing cells and a constant column (sample 4: NA with every partner)"""
    rng = np.random.default_rng(12)
    X = rng.standard_normal((30, 12))
    X[rng.random(X.shape) < 0.1] = np.nan
    X[:, 4] = 2.5
    names = [f"s{i}" for i in range(12)]
    labels = ["a", "b", "a", "c", "a", "b", "b", "a", "b", "a", "b", "a"]     # "c": a singleton
    return X, names, labels


def _full(X, names, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = api.ici_kendalltau(X, colnames=names, engine=OracleEngine(), **kw)
    return [np.asarray(full[key]) for key in ("cor", "raw", "pvalue", "taumax", "completeness")]


@pytest.mark.parametrize("kw", [{}, {"scale_max": False}, {"perspective": "local"}])
def test_front_end_with_classes(small, kw):
    X, names, labels = small
    cls = np.array([{"a": 0, "b": 1, "c": 2}[v] for v in labels])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = api.ici_kendalltau_quantiles(X, probs=PROBS, breaks=7, sample_classes=labels, colnames=names,
                                           engine=OracleEngine(), **kw)
    msgs = [str(x.message) for x in w if str(x.message) in _lib.REASON_WARNINGS.values()]
    assert len(msgs) == 11 and set(msgs) == {_lib.REASON_WARNINGS[_lib.REASON_SINGLE_UNIQUE]}
    out5 = _full(X, names, **kw)
    breaks = np.linspace(-1.0, 1.0, 8)
    q2, _order2, n_valid, n_na, hist, outside = brute_quantiles(out5, cls, PROBS, breaks)
    assert res["group"] == ["all", "within", "between"]
    assert np.array_equal(res["probs"], np.asarray(PROBS, dtype=np.float64))
    assert res["quantile_cor"].shape == res["quantile_raw"].shape == (3, len(PROBS))
    assert np.array_equal(bits(res["quantile_cor"]), bits(q2[0]))
    assert np.array_equal(bits(res["quantile_raw"]), bits(q2[1]))
    assert np.array_equal(res["n_valid"], n_valid) and np.array_equal(res["n_na"], n_na)
    assert n_na[0] == 11 and n_valid[0] == 66 - 11 and n_na[1] + n_na[2] == 11
    assert np.array_equal(res["breaks"], breaks) and res["counts"].shape == (3, 7)
    assert np.array_equal(res["counts"], hist)
    assert np.array_equal(res["n_below"], outside[:, 0]) and np.array_equal(res["n_above"], outside[:, 1])
    iu, ju = np.triu_indices(12, k=1)
    assert res["max_taumax"] == np.nanmax(out5[3][iu, ju])
    if not kw.get("scale_max", True):
        assert np.array_equal(bits(res["quantile_cor"]), bits(res["quantile_raw"]))


def test_front_end_one_group_and_optional_parts(small):
    X, names, _labels = small
    out5 = _full(X, names)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = api.ici_kendalltau_quantiles(X, colnames=names, engine=OracleEngine())
        no_hist = api.ici_kendalltau_quantiles(X, breaks=None, colnames=names, engine=OracleEngine())
        no_probs = api.ici_kendalltau_quantiles(X, probs=(), breaks=[-1.0, -0.1, 0.3, 1.0], colnames=names,
                                                engine=OracleEngine())
    q2, _o, n_valid, n_na, hist, outside = brute_quantiles(out5, None, (0, 0.25, 0.5, 0.75, 1), np.linspace(-1.0, 1.0, 201))
    assert res["group"] == ["all"] and res["quantile_raw"].shape == (1, 5) and res["counts"].shape == (1, 200)
    assert np.array_equal(bits(res["quantile_raw"]), bits(q2[1])) and np.array_equal(res["counts"], hist)
    assert np.array_equal(res["n_valid"], n_valid) and res["counts"].sum() == n_valid[0]
    assert no_hist["breaks"] is None and no_hist["counts"].shape == (1, 0) and no_hist["n_below"].tolist() == [0]
    assert np.array_equal(bits(no_hist["quantile_cor"]), bits(res["quantile_cor"]))
    assert no_probs["quantile_raw"].shape == (1, 0) and no_probs["counts"].shape == (1, 3)
    assert np.array_equal(no_probs["counts"], brute_quantiles(out5, None, (), [-1.0, -0.1, 0.3, 1.0])[4])


def test_argument_errors(small):
    X, names, labels = small
    eng = OracleEngine()
    with pytest.raises(ValueError, match="`sample_classes` must give one class per column"):
        api.ici_kendalltau_quantiles(X, sample_classes=["a"] * 3, colnames=names, engine=eng)
    with pytest.raises(ValueError, match="Colnames"):
        api.ici_kendalltau_quantiles(X, engine=eng)
    with pytest.raises(ValueError, match="No comparisons to do"):
        api.ici_kendalltau_quantiles(X[:, :1], colnames=names[:1], engine=eng)
    for bad in ((0.5, 1.5), (nan,), tuple([0.5] * 33)):
        with pytest.raises(ValueError, match="`probs`"):
            api.ici_kendalltau_quantiles(X, probs=bad, colnames=names, engine=eng)
    for bad in (0, 1025, [0.0], [0.0, 0.0, 1.0], [0.0, np.inf], [1.0, 0.0]):
        with pytest.raises(ValueError, match="`breaks`"):
            api.ici_kendalltau_quantiles(X, breaks=bad, colnames=names, engine=eng)


def test_engines_pass_their_flags_on():
    """an engine built with exact_int64=True asks for it in this entry as in topk, edges and class_medians"""
    seen = []

    class Recorder:
        def quantiles(self, *args):
            seen.append(args)
            return "result"

    for cls_ in (api.HipEngine, api.MultiHipEngine):
        eng = object.__new__(cls_)
        eng.ctx = eng._single = Recorder()
        eng.flags = _lib.FLAG_EXACT_INT64
        assert eng.quantiles("X", (0.5,), None, None, 1, None, "global", "two.sided", False, _lib.FLAG_TIMING, True) == "result"
        assert seen[-1] == ("X", (0.5,), None, None, 1, None, "global", "two.sided", False,
                            _lib.FLAG_EXACT_INT64 | _lib.FLAG_TIMING, True)


def test_exports():
    import icikendalltau_amd as pkg
    assert pkg.ici_kendalltau_quantiles is api.ici_kendalltau_quantiles
    src = open(os.path.join(ROOT, "include", "icikt.h")).read()
    defs = dict(re.findall(r"#define\s+(ICIKT_[A-Z0-9_]+)\s+\(?(-?\d+)u?\)?", src))
    assert int(defs["ICIKT_QUANTILE_MAX_PROBS"]) == _lib.QUANTILE_MAX_PROBS == 32
    assert int(defs["ICIKT_HIST_MAX_BINS"]) == _lib.HIST_MAX_BINS == 1024
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(icikt_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.EXPORTS)              # what tests/test_abi.py holds the library to
    for nm in ("icikt_quantiles_f64", "icikt_quantiles_in", "icikt_quantiles_csc"):
        assert nm in _lib.EXPORTS
        assert re.search(rf"\bint {nm}\s*\(", src), nm
    for f in ("icikt_quantiles.hip", "icikt_capi_quantiles.cpp"):
        assert os.path.join(ROOT, "icikendalltau_amd", "csrc", f) in _lib.SOURCES
    assert hasattr(api.HipEngine, "quantiles") and hasattr(api.MultiHipEngine, "quantiles")
    assert hasattr(_lib.Context, "quantiles")
