"""What tests/test_gpu_caller_stream.py relies on in its cases (tests/stream_cases.py), checked with the CPU oracle
alone: every pair of every case has an answer (reason 0), every pair's tau differs between the true and the decoy
matrix -- so a snapshot that equals the true answers cannot have been computed from the decoy, in whole or in part --,
and no reference value equals the sentinel the test fills its buffers with."""
import numpy as np
import pytest

from tests import stream_cases as sc


def _check(ref, decoy):
    for persp in ("global", "local"):
        out, cnt, rsn = ref[persp]
        dout, _dcnt, drsn = decoy[persp]
        assert out.shape == (sc.PAIRS, 4) and rsn.shape == (sc.PAIRS,)
        assert np.all(rsn == 0) and np.all(drsn == 0)
        assert np.all(np.isfinite(out)) and np.all(np.isfinite(dout))
        same = out[:, 0] == dout[:, 0]
        assert not same.any(), np.nonzero(same)[0]                     # all 28 pairs, no share left out
        assert not np.any(np.all(out == dout, axis=1))
        assert not np.any(out == sc.SENTINEL) and not np.any(cnt == int(sc.SENTINEL))
        assert not np.any(rsn == int(sc.SENTINEL))


def test_the_cases_are_the_documented_ones():
    assert sc.S == 8 and sc.PAIRS == 28 and sc.SENTINEL == -7.0
    assert {7168, 10000, 20000, 33000, 70000, 40, 700} <= set(sc.LENGTHS)
    assert set(sc.ALL_KINDS_AT) == {700, 10000, 70000}
    assert len(sc.CASES) == 2 * len(sc.LENGTHS)
    assert list(zip(sc.IU[:8], sc.JU[:8])) == [(0, j) for j in range(1, 8)] + [(1, 2)]      # combn order
    blocks = sc.combn_blocks()
    assert blocks[0][0] == 0 and blocks[-1][1] == sc.PAIRS and all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
    assert len({e - b for b, e in blocks}) > 1 and all(e > b for b, e in blocks)
    perm, pi, pj = sc.shuffled_pairs()
    assert sorted(perm) == list(range(sc.PAIRS)) and not np.array_equal(perm, np.arange(sc.PAIRS))
    ranges, alloc = sc.rank_ranges()
    assert ranges == [(0, 4), (4, 8), (8, 8)] and alloc == 12


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_case(case):
    X, D = sc.true_matrix(case), sc.decoy_matrix(case)
    assert X.shape == D.shape == (case.n, sc.S) and X.flags.f_contiguous
    for M in (X, D):
        rate = np.isnan(M).mean()
        assert abs(rate - sc.NAN_RATE) < 4.0 * np.sqrt(sc.NAN_RATE / M.size) + 1e-12, rate
    if case.variant == "tied":
        odd = X[:, 1::2]
        assert np.all(np.isnan(odd) | (np.round(odd * 3.0) / 3.0 == odd))
        assert len(np.unique(X[~np.isnan(X[:, 0]), 0])) == np.sum(~np.isnan(X[:, 0]))        # the even columns stay continuous
    _check(sc.reference(case), sc.decoy_reference(case))


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_float32_sources(variant):
    """the matrices of the icikt_convert_dev case: the same conditions on the values a float32 source carries"""
    case = sc.Case(700, variant)
    _check(sc.oracle_answers(sc.as_float32(sc.true_matrix(case))), sc.oracle_answers(sc.as_float32(sc.decoy_matrix(case))))
