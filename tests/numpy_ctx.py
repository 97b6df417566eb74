"""The library's engine-free numpy paths (icikendalltau_amd.api._*_numpy) behind the device context's method names, so
that the diagnostics / cor_fast checks of the GPU tests also run on the CPU (test infrastructure only)."""
import numpy as np

from icikendalltau_amd import api
from tests import diag_checker as dc


class NumpyCtx:
    def col_medians(self, X, na_rm=False, global_na=None):
        return api._col_medians_numpy(X, na_rm, dc.rule(X, global_na or ())[0])

    def censor_counts(self, X, global_na, cls, n_class, want_medians=False):
        tr, su, nex = api._censor_numpy(X, list(global_na), np.asarray(cls), n_class)
        med = api._col_medians_numpy(X, True, dc.rule(X, global_na)[0]) if want_medians else None
        return tr, su, nex, med

    def rank_order(self, X, global_na, cols, want_data=True):
        return api._rank_order_numpy(X, list(global_na), np.asarray(cols))

    def cor_pairs(self, X, pi, pj, method="pearson", pairwise=False):
        return api._cor_pairs_numpy(X, np.asarray(pi), np.asarray(pj), method, pairwise, "two.sided", False)
