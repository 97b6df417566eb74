"""cor_fast's Student-t p-values on the MI355X (``k_cor_epilogue``'s ``t_tail`` / ``cor_pt`` through
``icikt_cor_pairs_f64``) on a designed (n, rho) lattice (tests/cor_lattice.py) against the series at 400 digits
(tests/t_tail_exact.py), at the device's own returned rho: every Pearson p-value, and Spearman's with ties or at
n >= 1290.  The bars are those of tests/test_gpu_cor_fast.py: |d| <= 1e-10 everywhere, 1e-8 relative wherever the
reference is >= 1e-290, which only the named underflow points may escape.  Dense, and with six more rows the first
column lacks, so that the joint n and the sums come from the pairwise kernels.  The figures printed here are
recorded in profiles/cor_t_tail.md."""
import numpy as np
import pytest

from icikendalltau_amd import _lib
from tests import cor_lattice as L
from tests.t_tail_exact import ALTERNATIVES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("n", L.PEARSON_N)
def test_pearson_lattice(hip_ctx, n, pad):
    if n + pad > _lib.MAX_FEATURES_WIDE:         # at the cap the padded matrix has the cap's rows, the pairs six fewer
        n -= pad
    tg = L.pearson_targets(n)
    X, pi, pj = L.pearson_lattice(n, tg, pad)
    want_rho = np.array([t.rho for t in tg])
    designed = [not t.underflow for t in tg]
    for alternative in ALTERNATIVES:
        out, rsn = hip_ctx.cor_pairs(X, pi, pj, "pearson", bool(pad), alternative, False)
        assert (rsn == _lib.COR_OK).all() and (out[:, 2] == n).all()
        assert np.abs(out[:, 0] - want_rho).max() <= 1e-9
        for k, t in enumerate(tg):
            if abs(t.rho) == 1:                  # identical / negated columns: rho = +-1 exactly, p = 0 or 1
                assert out[k, 0] == t.rho
                assert out[k, 1] == (0.0 if L.on_tail_side(t.rho, alternative) else 1.0)
        checked, _, _ = L.compare_with_exact(out[:, 0], out[:, 1], n - 2, alternative, designed,
                                             f"device pearson pad={pad}")
        assert checked == sum(d and L.on_tail_side(t.rho, alternative) for d, t in zip(designed, tg))


@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("n,tied", L.SPEARMAN_CASES)
def test_spearman_lattice(hip_ctx, n, tied, pad):
    """The t branch of Spearman's p-value: ties (ICIKT_COR_TIES below n = 1290), or n >= 1290; df = n - 2, no
    continuity correction.  Every point is checked relatively."""
    X, pi, pj = L.spearman_lattice(n, tied, pad)
    for alternative in ALTERNATIVES:
        out, rsn = hip_ctx.cor_pairs(X, pi, pj, "spearman", bool(pad), alternative, False)
        assert (rsn == (_lib.COR_TIES if tied and n < 1290 else _lib.COR_OK)).all() and (out[:, 2] == n).all()
        checked, _, _ = L.compare_with_exact(out[:, 0], out[:, 1], n - 2, alternative, [True] * len(pi),
                                             f"device spearman tied={tied} pad={pad}")
        assert checked == sum(L.on_tail_side(float(r), alternative) for r in out[:, 0])
    L.assert_spearman_spread(out[:, 0], n)
