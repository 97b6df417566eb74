"""api.ici_kendalltau_cross on an engine without a cross method (the CPU oracle): the rectangle against the
[query, reference] block of ici_kendalltau on the stacked matrix, cor by its formula, the top-k lists against the
brute-force checker (tests/cross_checker.py), the error texts, the names and the CSR converter."""
import warnings

import numpy as np
import pytest

from icikendalltau_amd import _lib, api, formats
from tests.cross_checker import KEYS, assert_topk_same, bits, brute_cross_topk, max_taumax, rect_block
from tests.oracle_engine import OracleEngine
from tests.topk_checker import NA_REAL_BITS


def _data(Sq=3, Sr=5, n=40, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, Sq + Sr))
    X[rng.random((n, Sq + Sr)) < 0.08] = np.nan
    return X[:, :Sq].copy(), X[:, Sq:].copy(), [f"q{i}" for i in range(Sq)], [f"r{j}" for j in range(Sr)]


def _cross(Q, R, qn, rn, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return api.ici_kendalltau_cross(Q, R, query_names=qn, reference_names=rn, engine=OracleEngine(), **kw)


def _stacked_block(Q, R, **kw):
    """The [query, reference] block of ici_kendalltau(hstack, scale_max=False): all pairs of the stacked matrix."""
    S = Q.shape[1] + R.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = api.ici_kendalltau(np.hstack([Q, R]), colnames=[f"s{i}" for i in range(S)], scale_max=False,
                                  engine=OracleEngine(), **kw)
    return rect_block([full[key] for key in KEYS], Q.shape[1])


def _assert_rectangle(res, block, scale_max=True):
    for f, key in enumerate(KEYS[1:], start=1):
        assert np.array_equal(bits(res[key]), bits(block[f])), key
    mx = max_taumax(block)
    assert res["max_taumax"] == mx
    with np.errstate(invalid="ignore"):
        want = block[1] / mx if scale_max else block[1]
    assert np.array_equal(bits(res["cor"]), bits(want))


def _cases():
    Q, R, qn, rn = _data()
    yield "40 x (3 + 5)", Q, R, qn, rn
    Qc = Q.copy()
    Qc[:, 1] = 2.5
    yield "a constant query column", Qc, R, qn, rn
    Rb = R.copy()
    Rb[:, 3] = Q[:, 2]
    yield "a column in both sets", Q, Rb, qn, rn


@pytest.mark.parametrize("name", ["40 x (3 + 5)", "a constant query column", "a column in both sets"])
@pytest.mark.parametrize("scale_max", [True, False])
def test_rectangle_is_the_block_of_the_stacked_matrix(name, scale_max):
    Q, R, qn, rn = next(c[1:] for c in _cases() if c[0] == name)
    res = _cross(Q, R, qn, rn, k=4, scale_max=scale_max)
    block = _stacked_block(Q, R)
    _assert_rectangle(res, block, scale_max)
    rect5 = [np.asarray(res[key]) for key in KEYS]
    assert_topk_same(res["indices"], np.stack([res["topk_" + key] for key in KEYS]), res["n_valid"],
                     brute_cross_topk(rect5, 4))
    assert res["indices"].dtype == np.int32 and res["indices"].shape == (3, 4)


def test_local_perspective_and_alternative():
    Q, R, qn, rn = _data()
    kw = dict(perspective="local", alternative="greater", continuity=True)
    _assert_rectangle(_cross(Q, R, qn, rn, **kw), _stacked_block(Q, R, **kw))


def test_constant_query_column_has_no_partner():
    Q, R, qn, rn = _data()
    Q[:, 1] = 2.5
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = api.ici_kendalltau_cross(Q, R, k=6, query_names=qn, reference_names=rn, engine=OracleEngine())
    msgs = [str(x.message) for x in w if str(x.message) == _lib.REASON_WARNINGS[_lib.REASON_SINGLE_UNIQUE]]
    assert len(msgs) == R.shape[1]                       # once per pair of the constant column
    assert res["n_valid"].tolist() == [5, 0, 5]
    assert np.all(res["indices"][1] == -1) and np.all(res["indices"][:, 5] == -1)
    assert np.all(bits(res["topk_raw"][1]) == NA_REAL_BITS)
    assert all(nm is None for nm in res["neighbors"][1])


def test_a_shared_column_is_a_partner_like_any_other():
    Q, R, qn, rn = _data()
    R[:, 3] = Q[:, 2]
    res = _cross(Q, R, qn, rn, k=2)
    assert res["indices"][2, 0] == 3 and res["neighbors"][2, 0] == "r3"
    assert res["topk_raw"][2, 0] == np.asarray(res["raw"])[2, 3] == np.nanmax(np.asarray(res["raw"])[2])


def test_equal_raw_is_ordered_by_reference_index():
    Q, R, qn, rn = _data()
    R[:, 4] = R[:, 1]
    res = _cross(Q, R, qn, rn, k=5, return_matrix=False)
    assert "raw" not in res and "cor" not in res
    for q in range(3):
        row = res["indices"][q].tolist()
        assert row.index(4) == row.index(1) + 1, row
        assert bits(res["topk_raw"][q])[row.index(1)] == bits(res["topk_raw"][q])[row.index(4)]


def test_names_tables_and_keys():
    pd = pytest.importorskip("pandas")
    Q, R, qn, rn = _data()
    res = _cross(Q, R, qn, rn)
    assert "indices" not in res and "n_valid" not in res
    for key in KEYS:
        assert isinstance(res[key], pd.DataFrame) and res[key].shape == (3, 5)
        assert list(res[key].index) == qn and list(res[key].columns) == rn
    assert res["query_names"] == qn and res["reference_names"] == rn and res["run_time"] >= 0.0
    frames = _cross(pd.DataFrame(Q, columns=qn), pd.DataFrame(R, columns=rn), None, None, k=1)
    assert frames["neighbors"].shape == (3, 1) and set(frames["neighbors"][:, 0]) <= set(rn)
    assert np.array_equal(bits(frames["raw"]), bits(res["raw"]))
    # the same name on both sides is no conflict: the sets are separate
    same = _cross(Q, R, ["a", "b", "c"], ["a", "b", "c", "d", "e"], k=1)
    assert np.array_equal(bits(same["raw"]), bits(res["raw"]))


def test_empty_sides():
    Q, R, qn, rn = _data()
    res = _cross(Q[:, :0], R, [], rn, k=2)
    assert np.asarray(res["raw"]).shape == (0, 5) and res["indices"].shape == (0, 2) and res["max_taumax"] == -np.inf
    res = _cross(Q, R[:, :0], qn, [], k=2)
    assert np.asarray(res["raw"]).shape == (3, 0) and res["n_valid"].tolist() == [0, 0, 0]
    assert np.all(res["indices"] == -1) and np.all(bits(res["topk_cor"]) == NA_REAL_BITS)


@pytest.mark.parametrize("k", [0, 257, 2.5, True, "3"])
def test_bad_k_is_a_value_error(k):
    Q, R, qn, rn = _data()
    with pytest.raises(ValueError, match="`k` must be None or an integer in 1 .. 256"):
        api.ici_kendalltau_cross(Q, R, k=k, query_names=qn, reference_names=rn, engine=OracleEngine())


def test_front_end_refusals():
    Q, R, qn, rn = _data()
    with pytest.raises(ValueError, match="Colnames of `query`"):
        api.ici_kendalltau_cross(Q, R, reference_names=rn, engine=OracleEngine())
    with pytest.raises(ValueError, match="Colnames of `reference`"):
        api.ici_kendalltau_cross(Q, R, query_names=qn, engine=OracleEngine())
    with pytest.raises(ValueError, match="`query` has 39 rows .* `reference` has 40"):
        api.ici_kendalltau_cross(Q[:39], R, query_names=qn, reference_names=rn, engine=OracleEngine())
    with pytest.raises(ValueError, match="nothing to return"):
        api.ici_kendalltau_cross(Q, R, return_matrix=False, query_names=qn, reference_names=rn, engine=OracleEngine())
    with pytest.raises(TypeError, match="`reference` must be a numeric type"):
        api.ici_kendalltau_cross(Q, R.astype(str), query_names=qn, reference_names=rn, engine=OracleEngine())


def test_long_global_na_lists_are_masked_on_the_host():
    """More finite values than the device rule holds: the same result as masking both matrices beforehand."""
    rng = np.random.default_rng(9)
    Q = rng.integers(0, 60, size=(40, 3)).astype(np.float64)
    R = rng.integers(0, 60, size=(40, 5)).astype(np.float64)
    qn, rn = [f"q{i}" for i in range(3)], [f"r{j}" for j in range(5)]
    gna = tuple(float(v) for v in range(_lib.MASK_VALS + 3))
    res = _cross(Q, R, qn, rn, global_na=gna)
    Qm, Rm = Q.copy(), R.copy()
    Qm[np.isin(Q, gna)] = np.nan
    Rm[np.isin(R, gna)] = np.nan
    want = _cross(Qm, Rm, qn, rn, global_na=(float("nan"),))
    for key in ("raw", "pvalue", "taumax"):
        assert np.array_equal(bits(res[key]), bits(want[key])), key


def test_cross_topk_to_csr():
    pytest.importorskip("scipy")
    Q, R, qn, rn = _data()
    Q[:, 1] = np.nan
    res = _cross(Q, R, qn, rn, k=3)
    for value in ("cor", "raw"):
        g = formats.cross_topk_to_csr(res, value=value)
        assert g.shape == (3, 5)
        assert g.nnz == int(res["n_valid"].sum())
        dense = g.toarray()
        for q in range(3):
            m = res["n_valid"][q]
            assert np.array_equal(dense[q, res["indices"][q, :m]], res["topk_" + value][q, :m])
    assert formats.cross_topk_to_csr(res, n_reference=9).shape == (3, 9)
    with pytest.raises(ValueError):
        formats.cross_topk_to_csr(res, value="nope")
    with pytest.raises(ValueError, match="no top-k lists"):
        formats.cross_topk_to_csr(_cross(Q, R, qn, rn))
