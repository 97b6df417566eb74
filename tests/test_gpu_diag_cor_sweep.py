"""Seeded random sweep of the missing-value diagnostics and cor_fast on the MI355X (tests/diag_cor_cases.py): lengths
at the kernels' boundaries up to 262 144 rows, short-and-wide shapes past the 2 048-column cap, tied, infinite, signed
zero, extreme and all-missing values, global_na sets; every result against the CPU references.  A failing input is
written under the test's tmp_path."""
import numpy as np
import pytest

from tests import diag_cor_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,cases", [(101, 40), (102, 40)])
def test_diag_cor_random_sweep(hip_ctx, seed, cases, tmp_path):
    rng = np.random.default_rng(seed)
    bad = [msg for case in range(cases) if (msg := diag_cor_cases.one_case(hip_ctx, rng, case, str(tmp_path)))]
    assert not bad, "\n".join(bad)
