"""Spearman's exact-test p-value on the MI355X (``k_cor_epilogue``'s ``prho`` through ``icikt_cor_pairs_f64``) against
the exact permutation distribution of S (tests/spearman_exact.py), from data to p: the Edgeworth branch at n = 10, 11,
13, 16 within AS 89's own error, the uploaded table at n = 5, 9 to 1e-12 relative, dense and with the joint rows found
by ``k_cor_spearman_pw``; and at n = 1289, the last n of the branch, against the t tail at the device's own rho."""
import math

import numpy as np
import pytest

from icikendalltau_amd import _lib
from tests import spearman_exact as SE
from tests.cor_checker import check_pairs, t_pvalue

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [5, 9, 10, 11, 13, 16])
def test_dense_ladder(hip_ctx, n):
    assert _lib.COR_OK == 0
    SE.assert_ladder_within_as89(SE.ladder_errors(hip_ctx.cor_pairs, n), n, "device, dense")


@pytest.mark.parametrize("n", [5, 9, 10, 11, 13, 16])
def test_pairwise_ladder(hip_ctx, n):
    """Six more rows where column 0 is NaN: the joint n, and with it the branch and the series' b = 1 / n, come from
    the pairwise kernel."""
    SE.assert_ladder_within_as89(SE.ladder_errors(hip_ctx.cor_pairs, n, pad=6), n, "device, pairwise")


def test_large_end_follows_the_t_tail(hip_ctx):
    """n = 1289: the series and the t approximation describe the same distribution, 2.6e-5 apart at most over
    |z| <= 6.  1e-4 leaves a margin of 4; overflow or a wrong scale in n^3 shows at 1e-2 and more."""
    n = 1289
    X = SE.factor_columns(n)
    K = X.shape[1] - 1
    pi, pj = np.zeros(K, dtype=np.int32), np.arange(1, K + 1, dtype=np.int32)
    want, warned = check_pairs(X, pi, pj, "spearman", False)
    assert not warned
    z = want[:, 0] * math.sqrt(n - 1)
    assert z.min() < -4.5 and z.max() > 4.5 and (np.abs(z) < 1).any()      # both tails and the centre
    for alt in ("less", "greater"):
        out, rsn = hip_ctx.cor_pairs(X, pi, pj, "spearman", False, alt, False)
        assert (rsn == _lib.COR_OK).all() and (out[:, 2] == n).all()
        np.testing.assert_allclose(out[:, 0], want[:, 0], atol=1e-12, rtol=0)
        t = out[:, 0] / np.sqrt((1 - out[:, 0] ** 2) / (n - 2))
        pt = np.array([t_pvalue(float(v), n - 2, alt) for v in t])
        print(f"n = {n} {alt}: worst |p - t tail| = {np.abs(out[:, 1] - pt).max():.3g}, p from {out[:, 1].min():.3g}")
        np.testing.assert_allclose(out[:, 1], pt, atol=1e-4, rtol=0)
