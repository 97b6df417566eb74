"""Host-side mirror of the reference's R interface for the all-pairs ICI-Kendall-tau path.

R is not available in the build image, so the host logic the reference keeps in R
(R/kendalltau.R:96-308,357-421,563-629; R/utils.R:1-66) is mirrored here in Python with the same
function names, argument names, defaults, return shapes and error / warning texts, on top of the
C ABI (include/icikt.h).  The R glue a maintainer would use instead lives in icikendalltau_amd/r/.

Every number is computed by the HIP kernels through ``engine`` (default: the MI355X engine, which
raises when no GPU is usable -- there is no CPU fallback).  ``engine`` exists so the sharding /
gather / reshape logic can be exercised in CPU-only tests with a checker engine.
"""
from __future__ import annotations

import math
import time
from fractions import Fraction
import warnings
from typing import Sequence

import numpy as np

from . import _lib

try:  # pandas is the natural carrier of R's data.frame / dimnames; numpy-only callers still work
    import pandas as pd
except Exception:  # pragma: no cover
    pd = None


# --------------------------------------------------------------------------------------------------
# engines
# --------------------------------------------------------------------------------------------------
class HipEngine:
    """Runs pair lists on one MI355X through libicikt_hip.so."""

    name = "hip"

    def __init__(self, device: int | None = None, exact_int64: bool = False):
        self.ctx = _lib.default_context(device)
        self.flags = _lib.FLAG_EXACT_INT64 if exact_int64 else 0

    def pairs(self, X, pi, pj, perspective, alternative, continuity):
        out, _cnt, rsn = self.ctx.pairs(X, pi, pj, perspective, alternative, continuity, self.flags,
                                        want_counts=False)
        return out, rsn

    def pairs_counts(self, X, pi, pj, perspective, alternative, continuity):
        """pairs() plus the integer counts record (dict of arrays keyed by _lib.CNT_FIELDS)."""
        out, cnt, rsn = self.ctx.pairs(X, pi, pj, perspective, alternative, continuity, self.flags, want_counts=True)
        return out, rsn, {k: cnt[:, i] for i, k in enumerate(_lib.CNT_FIELDS)}

    def missingness(self, X, pi, pj):
        return self.ctx.missingness(X, pi, pj)

    def matrix(self, data_matrix, global_na, pi, pj, perspective, alternative, continuity, scale_max, diag_good):
        """The whole of ici_kendalltau() below its argument checks in one library call (icikt_matrix_f64 /
        icikt_matrix_multi_f64): exclusion rule, pair kernels and scale_and_reshape on the device.  Returns
        (out5 [5, S, S]: cor, raw, pvalue, taumax, completeness; keep [S, n_feat] bool; pairs per reason code [5])."""
        return self.ctx.matrix(data_matrix, global_na, pi, pj, perspective, alternative, continuity, self.flags,
                               scale_max, diag_good, want_keep=True)

    def topk(self, data_matrix, k, global_na=None, perspective="global", alternative="two.sided", continuity=False,
             flags=0, scale_max=True):
        """Every sample's k best partners, selected on the device (icikt_topk_f64): Context.topk's contract."""
        return self._select_ctx().topk(data_matrix, k, global_na, perspective, alternative, continuity,
                                       self.flags | flags, scale_max)

    def cross(self, query, reference, k=None, want_matrix=True, global_na=None, perspective="global",
              alternative="two.sided", continuity=False, flags=0, scale_max=True):
        """The query x reference rectangle, its matrices and / or every query's k best reference columns, on the device
        (icikt_cross_f64): Context.cross' contract."""
        return self._select_ctx().cross(query, reference, k, want_matrix, global_na, perspective, alternative,
                                        continuity, self.flags | flags, scale_max)

    def prepare_reference(self, reference, query_capacity, global_na=None):
        """A reference uploaded and pre-passed once, on a context of ITS OWN on the device of the selection entries
        (icikt_ref_prepare_f64) -- no other entry of this engine can displace it.  Returns the _lib.Context: its
        cross_prepared() takes the batches, its close() frees the reference."""
        ctx = _lib.Context(self._select_ctx().device)
        try:
            ctx.prepare_reference(reference, query_capacity, global_na, self.flags)
        except Exception:
            ctx.close()
            raise
        return ctx

    def edges(self, data_matrix, min_raw=None, max_pvalue=None, min_completeness=None, absolute=False, max_edges=0,
              global_na=None, perspective="global", alternative="two.sided", continuity=False, flags=0, scale_max=True):
        """Every pair past the bounds, compacted on the device (icikt_edges_f64): Context.edges' contract."""
        return self._select_ctx().edges(data_matrix, min_raw, max_pvalue, min_completeness, absolute, max_edges,
                                        global_na, perspective, alternative, continuity, self.flags | flags, scale_max)

    def class_medians(self, data_matrix, cls=None, n_class=1, global_na=None, perspective="global",
                      alternative="two.sided", continuity=False, flags=0, scale_max=True):
        """Every sample's median over its class, reduced on the device (icikt_class_medians_f64): Context.class_medians'
        contract."""
        return self._select_ctx().class_medians(data_matrix, cls, n_class, global_na, perspective, alternative,
                                                continuity, self.flags | flags, scale_max)

    def class_matrix(self, data_matrix, cls=None, n_class=1, global_na=None, perspective="global",
                     alternative="two.sided", continuity=False, flags=0, scale_max=True):
        """Every sample's median to every class, reduced on the device (icikt_class_matrix_f64): Context.class_matrix's
        contract."""
        return self._select_ctx().class_matrix(data_matrix, cls, n_class, global_na, perspective, alternative,
                                               continuity, self.flags | flags, scale_max)

    def quantiles(self, data_matrix, probs=(), breaks=None, cls=None, n_class=1, global_na=None, perspective="global",
                  alternative="two.sided", continuity=False, flags=0, scale_max=True):
        """Exact quantiles and a histogram of raw over all pairs, reduced on the device (icikt_quantiles_f64):
        Context.quantiles' arguments and result."""
        return self._select_ctx().quantiles(data_matrix, probs, breaks, cls, n_class, global_na, perspective,
                                            alternative, continuity, self.flags | flags, scale_max)

    def padjust(self, data_matrix, method, alpha, max_table=0, global_na=None, perspective="global",
                alternative="two.sided", continuity=False, flags=0):
        """R's p.adjust over the p-values of all pairs, on the device (icikt_padjust_f64): Context.padjust's arguments
        and result."""
        return self._select_ctx().padjust(data_matrix, method, alpha, max_table, global_na, perspective, alternative,
                                          continuity, self.flags | flags)

    def mst(self, data_matrix, min_raw=None, global_na=None, perspective="global", alternative="two.sided",
            continuity=False, flags=0, scale_max=True):
        """The maximum spanning forest under raw, found on the device (icikt_mst_f64): Context.mst's contract."""
        return self._select_ctx().mst(data_matrix, min_raw, global_na, perspective, alternative, continuity,
                                      self.flags | flags, scale_max)

    def hclust(self, data_matrix, method="complete", min_raw=None, global_na=None, perspective="global",
               alternative="two.sided", continuity=False, flags=0, scale_max=True):
        """Complete, average or single linkage under raw, run on the device (icikt_hclust_f64): Context.hclust's
        contract."""
        return self._select_ctx().hclust(data_matrix, method, min_raw, global_na, perspective, alternative, continuity,
                                         self.flags | flags, scale_max)

    def anosim(self, data_matrix, cls=None, n_class=1, perm_cls=None, global_na=None, perspective="global",
               alternative="two.sided", continuity=False, flags=0):
        """ANOSIM's rank sums of the observed labelling and of every permutation, on the device (icikt_anosim_f64):
        Context.anosim's arguments and result."""
        return self._select_ctx().anosim(data_matrix, cls, n_class, perm_cls, global_na, perspective, alternative,
                                         continuity, self.flags | flags)

    def permanova(self, data_matrix, cls=None, n_class=1, perm_cls=None, global_na=None, perspective="global",
                  alternative="two.sided", continuity=False, flags=0):
        """PERMANOVA's fixed-point sums per class of the observed labelling and of every permutation, on the device
        (icikt_permanova_f64): Context.permanova's arguments and result."""
        return self._select_ctx().permanova(data_matrix, cls, n_class, perm_cls, global_na, perspective, alternative,
                                            continuity, self.flags | flags)

    def permdisp(self, data_matrix, cls=None, n_class=1, global_na=None, perspective="global", alternative="two.sided",
                 continuity=False, flags=0):
        """PERMDISP's fixed-point sums of every sample to every class, on the device (icikt_permdisp_f64):
        Context.permdisp's arguments and result."""
        return self._select_ctx().permdisp(data_matrix, cls, n_class, global_na, perspective, alternative, continuity,
                                           self.flags | flags)

    def pcoa(self, data_matrix, k=10, tol=1e-8, max_basis=None, seed=0, return_gower=False, global_na=None,
             perspective="global", alternative="two.sided", continuity=False, flags=0):
        """The k largest eigenpairs of the Gower-centred table of (1 - raw)^2, found on the device (icikt_pcoa_f64):
        Context.pcoa's arguments and result."""
        return self._select_ctx().pcoa(data_matrix, k, tol, max_basis, seed, return_gower, global_na, perspective,
                                       alternative, continuity, self.flags | flags)

    def mantel(self, data_matrix, other, method="pearson", perms=None, global_na=None, perspective="global",
               alternative="two.sided", continuity=False, flags=0):
        """The Mantel test's integer sums against another matrix, of the identity and of every permutation, on the
        device (icikt_mantel_f64): Context.mantel's arguments and result."""
        return self._select_ctx().mantel(data_matrix, other, method, perms, global_na, perspective, alternative,
                                         continuity, self.flags | flags)

    def cor_pairs(self, X, pi, pj, method, pairwise, alternative, continuity):
        """cor_fast's pairs on the device (icikt_cor_pairs_f64): (out3: rho, p-value, n_values; reasons)."""
        return self.ctx.cor_pairs(X, pi, pj, method, pairwise, alternative, continuity)

    def col_medians(self, X, na_rm):
        """calculate_matrix_medians on the device (icikt_col_medians_f64)."""
        return self._diag_ctx().col_medians(X, na_rm)

    def censor_counts(self, X, global_na, cls, n_class):
        """test_left_censorship's per-class counts on the device (icikt_censor_counts_f64): (trials, success,
        n_excluded)."""
        trials, success, n_ex, _med = self._diag_ctx().censor_counts(X, global_na, cls, n_class)
        return trials, success, n_ex

    def rank_order(self, X, global_na, cols):
        """rank_order_data of one class on the device (icikt_rank_order_f64)."""
        return self._diag_ctx().rank_order(X, global_na, cols)

    def _diag_ctx(self):
        return self.ctx

    def _select_ctx(self):
        """The context the nine selection entries (topk ... anosim above) run on."""
        return self.ctx

    def pairs_complete(self, X, pi, pj):
        """kt_fast(use = "pairwise.complete.obs") on the device: (out4, reasons)."""
        out, _cnt, rsn = self.ctx.pairs_complete(X, pi, pj, "two.sided", False, self.flags)
        return out, rsn

    def pairs_block_dev(self, X, pi, pj, begin, end, n_each, perspective, alternative, continuity, dist, device,
                        via_host):
        """This rank's block [begin, end) of a pair list under torch.distributed: column-sharded pre-pass
        (sharding.ShardedPrepass; every rank falls back to the whole pre-pass together if it cannot be set up), then
        K1 + K2 into torch buffers on `device`, padded to n_each rows for the gather."""
        import torch
        from . import sharding
        ctx = self.ctx
        Xf = np.asfortranarray(X, dtype=np.float64)
        S = Xf.shape[1]
        with torch.cuda.device(device):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)  # one stream orders kernels and collectives
            try:
                sp = sharding.ShardedPrepass(ctx, dist, device, via_host)
                if not sp.setup(S, lambda c0, c1, alloc, fl: ctx.prepare_cols(Xf, c0, c1, alloc, fl),
                                sync=torch.cuda.synchronize):
                    ctx.prepare_cols(Xf, 0, S, S, 0)
                self.pre_pass = sp.mode
                out_l = torch.full((n_each, 4), float("nan"), dtype=torch.float64, device=device)
                rsn_l = torch.zeros(n_each, dtype=torch.int32, device=device)
                ctx.set_pairs(pi[begin:end], pj[begin:end])
                if end > begin:
                    ctx.run_dev(_lib.PERSPECTIVE[perspective], _lib.ALTERNATIVE.get(alternative, _lib.ALT_OTHER),
                                continuity, self.flags, out_l.data_ptr(), None, rsn_l.data_ptr())
                torch.cuda.synchronize()
            finally:
                ctx.use_own_stream()
        return out_l, rsn_l


class MultiHipEngine(HipEngine):
    """Runs pair lists on several MI355X behind ONE library call (icikt_pairs_multi_f64): one host thread per
    GPU inside the library, column-sharded pre-pass, RCCL all-gather / gather over xGMI.  This is what an R
    caller's `n_gpu` argument selects (icikendalltau_amd/r/icikt_mi355x.R); with torch.distributed ranks use
    HipEngine per rank instead."""

    name = "hip-multi"

    def __init__(self, devices=None, n_gpu: int | None = None, exchange: str = "auto", exact_int64: bool = False):
        self.ctx = _lib.MultiContext(devices, n_gpu, exchange)
        self._single = None
        self.flags = _lib.FLAG_EXACT_INT64 if exact_int64 else 0

    def _one(self):
        if self._single is None:
            self._single = _lib.default_context(self.ctx.devices[0])
        return self._single

    def missingness(self, X, pi, pj):  # a bitset popcount: one device is plenty
        return self._one().missingness(X, pi, pj)

    def _diag_ctx(self):  # the missing-value diagnostics run on one device
        return self._one()

    def _select_ctx(self):  # so do the selection entries: their folds, selects, sorts and rounds
        return self._one()

    def cor_pairs(self, X, pi, pj, method, pairwise, alternative, continuity):  # cor_fast runs on one device
        return self._one().cor_pairs(X, pi, pj, method, pairwise, alternative, continuity)

    def pairs_complete(self, X, pi, pj):  # kt_fast's per-pair masking path exists on one device only
        out, _cnt, rsn = self._one().pairs_complete(X, pi, pj, "two.sided", False, self.flags)
        return out, rsn


def _default_engine():
    return HipEngine()


_multi_engines: dict = {}


def _multi_engine(n_gpu, devices):
    """One MultiHipEngine per device list: RCCL communicators are expensive to create."""
    devs = tuple(int(d) for d in devices) if devices is not None else tuple(range(int(n_gpu)))
    if devs not in _multi_engines:
        _multi_engines[devs] = MultiHipEngine(devices=list(devs))
    return _multi_engines[devs]


# --------------------------------------------------------------------------------------------------
# ici_kt: one pair (R/RcppExports.R:62-64 -> src/kendallc.cpp:166)
# --------------------------------------------------------------------------------------------------
class IciKtResult(tuple):
    """Named numeric(4): c(tau, pvalue, tau_max, completeness) (src/kendallc.cpp:171-172)."""

    names = ("tau", "pvalue", "tau_max", "completeness")

    def __new__(cls, values):
        return super().__new__(cls, (float(v) for v in values))

    def __getitem__(self, key):
        if isinstance(key, str):
            return super().__getitem__(self.names.index(key))
        return super().__getitem__(key)

    tau = property(lambda self: self[0])
    pvalue = property(lambda self: self[1])
    tau_max = property(lambda self: self[2])
    completeness = property(lambda self: self[3])

    def __repr__(self):
        return "IciKtResult(" + ", ".join(f"{n}={v!r}" for n, v in zip(self.names, self)) + ")"


def _warn_reason(reason: int):
    msg = _lib.REASON_WARNINGS.get(int(reason))
    if msg:
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def ici_kt(x, y, perspective="local", alternative="two.sided", continuity=False, output="simple", engine=None):
    """Information-content-informed Kendall tau-b of two vectors (NaN = missing).

    Same defaults as the reference (src/kendallc.cpp:166).  Any ``output`` other than "simple" prints the
    reference's report (src/kendallc.cpp:342-363: same labels, ``std::to_string`` formatting) from the counts
    record of the pair; ``ici_kt_counts`` returns those integers instead of printing them.
    Vectors of up to 65 535 rows (``_lib.MAX_FEATURES``) run the tuned kernels; up to 262 144
    (``_lib.MAX_FEATURES_WIDE``) a plain 32-bit path in exact integer arithmetic; longer ones are refused with an
    error that names the limit.
    """
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    if x.shape[0] != y.shape[0]:
        raise ValueError("'X' and 'Y' are not the same length!")  # src/kendallc.cpp:168-170
    if perspective not in ("local", "global"):
        # the reference treats any string other than "local" as global (kendallc.cpp:180)
        perspective = "global"
    eng = engine or _default_engine()
    X = np.empty((x.shape[0], 2), dtype=np.float64, order="F")
    X[:, 0] = x
    X[:, 1] = y
    i0, i1 = np.array([0], np.int32), np.array([1], np.int32)
    if output != "simple" and hasattr(eng, "pairs_counts"):
        out, rsn, cnt = eng.pairs_counts(X, i0, i1, perspective, alternative, continuity)
        if rsn[0] == 0:  # the reference returns before its report in every NA case
            print(_ici_kt_report(x, y, perspective, continuity, out[0], {k: int(v[0]) for k, v in cnt.items()}), end="")
    else:
        out, rsn = eng.pairs(X, i0, i1, perspective, alternative, continuity)
    _warn_reason(rsn[0])
    return IciKtResult(out[0])


def _na_rm(a: np.ndarray) -> np.ndarray:
    """The non-missing values of `a`.  NOT np.nanmax / np.nanmin: R's NA_real_ -- the pattern the library returns for a
    pair without a result, and what a matrix read from an .rda file holds -- is a SIGNALLING NaN, and the C fmax / fmin
    behind numpy's NaN-skipping reductions answer NaN for one (the running maximum is lost wherever such a cell meets
    the scalar tail of the reduction)."""
    a = np.asarray(a)
    return a[~np.isnan(a)]


def _ici_kt_report(x, y, perspective, continuity, out4, k) -> str:
    """The text ici_kt(output != "simple") writes to Rcout (src/kendallc.cpp:342-363), rebuilt from the counts
    record: integers print as integers, doubles as std::to_string prints them ("%f")."""
    keep = ~(np.isnan(x) & np.isnan(y)) if perspective == "local" else np.ones(x.shape[0], bool)
    x2, y2 = x[keep].copy(), y[keep].copy()
    min_x, min_y = _na_rm(x2).min() - 0.1, _na_rm(y2).min() - 0.1    # :214-215
    x2[np.isnan(x2)] = min_x
    y2[np.isnan(y2)] = min_y
    sum_obs = len(np.unique(np.stack([x2, y2], axis=1), axis=0)) + 1  # joint runs + 1 (:261-263)
    n, tot = k["n"], k["tot"]
    m = n * (n - 1)
    ld = np.longdouble
    con_minus_dis = ld(tot) - k["xtie"] - k["ytie"] + k["ntie"] - 2 * k["dis"]
    var = (ld(m * (2 * n + 5)) - k["x1"] - k["y1"]) / 18 + ld(2.0 * k["xtie"] * k["ytie"]) / m + \
        ld(float(k["x0"]) * float(k["y0"])) / ld(9 * m * (n - 2)) if n > 2 else ld("nan")
    s_adj = ld(out4[0]) * np.sqrt(ld(m // 2 - k["xtie"]) * ld(m // 2 - k["ytie"]))
    if continuity:
        s_adj = np.sign(s_adj) * (abs(s_adj) - 1)
    z_b = s_adj / np.sqrt(var)
    f = lambda v: f"{float(v):f}"  # noqa: E731
    rows = [("min_x: ", f(min_x)), ("min_y: ", f(min_y)), ("n_entry: ", str(n)), ("missingness: ", str(k["missing"])),
            ("completeness: ", f(out4[3])), ("tot: ", str(tot)), ("sum_obs: ", str(sum_obs)), ("dis: ", str(k["dis"])),
            ("con_minus_dis (k_numerator): ", f(con_minus_dis)), ("n_tie: ", f(k["ntie"])), ("m: ", str(m)),
            ("x_tie: ", f(k["xtie"])), ("y_tie: ", f(k["ytie"])), ("s_adjusted: ", f(s_adj)), ("var: ", f(var)),
            ("z_b: ", f(z_b)), ("tau: ", f(out4[0])), ("tau_max:", f(out4[2])), ("pvalue: ", f(out4[1]))]
    return "".join(a + b + "\n" for a, b in rows)


def ici_kt_counts(x, y, perspective="local", device=None, exact_int64=False):
    """The integer counts ici_kt(..., output != "simple") prints (src/kendallc.cpp:342-363)."""
    ctx = _lib.default_context(device)
    out, cnt, rsn = ctx.pair(x, y, perspective, flags=_lib.FLAG_EXACT_INT64 if exact_int64 else 0)
    return cnt, rsn


# --------------------------------------------------------------------------------------------------
# input checks (R/utils.R:1-66)
# --------------------------------------------------------------------------------------------------
def _densify(A):
    """A sparse matrix as the dense one it stands for (toarray(): absent cells are 0), O(n_feat * n_samp) on the host."""
    return A.toarray() if hasattr(A, "toarray") else _lib.csc_view(A).toarray()


def _as_matrix(data_matrix, colnames, arg, keep_dtype=False, keep_sparse=False):
    """check_if_colnames_null / transform_to_matrix / check_if_numeric.  keep_dtype: a float32, int32 or int64 matrix
    stays what it is (a HipEngine's context reads it where it lies, _for_engine); everything else is float64.
    keep_sparse: a sparse matrix (scipy.sparse, or anything _lib.is_sparse takes) stays what it is too -- a HipEngine's
    context reads its CSC arrays where they lie (_lib.csc_view) -- after the same checks; without it it is densified."""
    if _lib.is_sparse(data_matrix):
        if colnames is None:
            raise ValueError(f"Colnames of `{arg}` must be be specified.")
        kind = np.asarray(getattr(data_matrix, "data", np.zeros(0))).dtype.kind
        if kind not in "fiub":
            raise TypeError(f"`{arg}` must be a numeric type.")
        colnames = [str(c) for c in colnames]
        if len(colnames) != data_matrix.shape[1]:
            raise ValueError("length of colnames does not match the number of columns")
        if keep_sparse:
            return data_matrix, colnames
        data_matrix = _densify(data_matrix)
    if pd is not None and isinstance(data_matrix, pd.DataFrame):
        print(f"i `{arg}` is a data.frame, converting to matrix ...")  # R/utils.R:53-57
        if colnames is None:
            colnames = [str(c) for c in data_matrix.columns]
        data_matrix = data_matrix.to_numpy()
    arr = np.asarray(data_matrix)
    if colnames is None:
        raise ValueError(f"Colnames of `{arg}` must be be specified.")  # R/utils.R:29-34 (sic)
    if arr.dtype.kind not in "fiu":
        raise TypeError(f"`{arg}` must be a numeric type.")  # R/utils.R:42-47
    if arr.ndim != 2:
        raise ValueError(f"`{arg}` must be a 2-D matrix (features x samples)")
    colnames = [str(c) for c in colnames]
    if len(colnames) != arr.shape[1]:
        raise ValueError("length of colnames does not match the number of columns")
    if keep_dtype and arr.dtype in _lib.DTYPES:
        return arr, colnames
    return np.asarray(arr, dtype=np.float64), colnames


def _for_engine(X, eng, fortran=True):
    """The matrix as an engine takes it.  A HipEngine's context reads float64, float32, int32 and int64 matrices of
    either memory order where they lie (_lib.input_view: no host copy); every other engine gets the float64 matrix it
    always got."""
    if _lib.is_sparse(X):
        # (one context reads the CSC arrays where they lie; the multi-device entries and every other engine take the
        #  dense matrix)
        if isinstance(eng, HipEngine) and not isinstance(eng, MultiHipEngine):
            return X
        X = _densify(X)
    if isinstance(eng, HipEngine):
        return X
    return np.asfortranarray(X, dtype=np.float64) if fortran else np.asarray(X, dtype=np.float64)


def setup_missing_matrix(data_matrix: np.ndarray, global_na) -> np.ndarray:
    """Logical exclude_loc (R/utils.R:1-23), in the memory order of the matrix (no transposing copies)."""
    vals = [] if global_na is None else list(np.atleast_1d(np.asarray(global_na, dtype=np.float64)))
    has_nan = any(math.isnan(v) for v in vals)
    has_inf = any(math.isinf(v) for v in vals)
    vals = [v for v in vals if not (math.isnan(v) or math.isinf(v))]
    if has_nan and has_inf:
        exclude = ~np.isfinite(data_matrix)  # one pass for NA and Inf
    elif has_nan:
        exclude = np.isnan(data_matrix)
    elif has_inf:
        exclude = np.isinf(data_matrix)
    else:
        exclude = np.zeros_like(data_matrix, dtype=bool)
    for v in vals:
        with np.errstate(invalid="ignore"):
            exclude |= (data_matrix == v)
    return exclude


def _masked_fortran(data_matrix: np.ndarray, exclude_loc: np.ndarray) -> np.ndarray:
    """exclude_data[exclude_loc] = NA (R/kendalltau.R:120-121) as a column-major float64 matrix."""
    out = np.array(data_matrix, dtype=np.float64, order="F", copy=True)
    out[exclude_loc] = np.nan
    return out


# --------------------------------------------------------------------------------------------------
# setup_comparisons (R/kendalltau.R:181-278)
# --------------------------------------------------------------------------------------------------
def _is_vector_like(obj):
    if isinstance(obj, (str, int, float, np.integer, np.floating)):
        return True
    if isinstance(obj, np.ndarray):
        return obj.ndim <= 1
    if isinstance(obj, (list, tuple)):
        return all(isinstance(v, (str, int, float, np.integer, np.floating)) for v in obj)
    return False


def _r_str(v) -> str:
    if isinstance(v, (float, np.floating)) and float(v).is_integer():
        return str(int(v))  # as.character(1) == "1"
    return str(v)


def _recycle(a: Sequence, n: int):
    return [a[i % len(a)] for i in range(n)]


def _no_comparisons(include_arg="include_only"):
    """The refusal of a call without a pair to compute (R/kendalltau.R:240-247)."""
    return ValueError(f"No comparisons to do. Check the list of column names in `{include_arg}` vs those in the samples.")


def _need_pairs(n_sample):
    """All pairs of the upper triangle: fewer than two samples have none."""
    if n_sample < 2:
        raise _no_comparisons()


def setup_comparisons(samples, include_only=None, diag_good=True, ncore=1, include_arg="include_only"):
    """Pair list in utils::combn order with include_only filtering; returns (i, j, core) 0-based arrays."""
    n_sample = len(samples)
    iu, ju = np.triu_indices(n_sample, k=1)  # row-major upper triangle == combn(n, 2) order
    pi = iu.astype(np.int32)
    pj = ju.astype(np.int32)
    if not diag_good:  # self comparisons appended after all pairs (R/kendalltau.R:191-194)
        d = np.arange(n_sample, dtype=np.int32)
        pi = np.concatenate([pi, d])
        pj = np.concatenate([pj, d])
    names = np.asarray(samples, dtype=object)

    if include_only is not None:
        if pd is not None and isinstance(include_only, pd.DataFrame):
            include_only = [include_only[c].tolist() for c in include_only.columns]
        elif isinstance(include_only, dict):
            include_only = list(include_only.values())
        if _is_vector_like(include_only):
            inc = {_r_str(v) for v in np.atleast_1d(np.asarray(include_only, dtype=object))}
            col_in = np.fromiter((nm in inc for nm in names), dtype=bool, count=n_sample)   # per SAMPLE, not per pair
            keep = col_in[pi] | col_in[pj]  # R/kendalltau.R:210-212
        elif isinstance(include_only, (list, tuple)):
            if len(include_only) == 2:
                l1 = [_r_str(v) for v in np.atleast_1d(np.asarray(include_only[0], dtype=object))]
                l2 = [_r_str(v) for v in np.atleast_1d(np.asarray(include_only[1], dtype=object))]
                m = max(len(l1), len(l2))
                l1r, l2r = _recycle(l1, m), _recycle(l2, m)  # paste0 recycles
                # "a-b" strings of the reference (:213-229) as index pairs: a listed name that is no sample matches
                # nothing; names holding "-" could make two different name pairs paste to one string -- those lists
                # keep the reference's string comparison
                if any("-" in str(nm) for nm in names) or any("-" in v for v in l1r + l2r):
                    allowed = {f"{a}-{b}" for a, b in zip(l1r, l2r)} | {f"{b}-{a}" for a, b in zip(l1r, l2r)}
                    keep = np.fromiter((f"{names[i]}-{names[j]}" in allowed for i, j in zip(pi, pj)), dtype=bool,
                                       count=len(pi))
                else:
                    index = {str(nm): k for k, nm in reversed(list(enumerate(names)))}   # first occurrence wins
                    ia = np.array([index.get(a, -1) for a in l1r], dtype=np.int64)
                    ib = np.array([index.get(b, -1) for b in l2r], dtype=np.int64)
                    ok = (ia >= 0) & (ib >= 0)
                    ia, ib = ia[ok], ib[ok]
                    codes = np.concatenate([ia * n_sample + ib, ib * n_sample + ia])
                    keep = np.isin(pi.astype(np.int64) * n_sample + pj, codes)
            else:
                raise ValueError(
                    f"`{include_arg}` must be a vector, a data.frame with two columns, or list of two vectors. "
                    f"Currently, `length({include_arg})` returns {len(include_only)}")  # R/kendalltau.R:230-236
        else:
            raise ValueError(f"`{include_arg}` must be a vector, a data.frame with two columns, or list of two vectors.")
        pi, pj = pi[keep], pj[keep]

    n_todo = len(pi)
    if n_todo == 0:
        raise _no_comparisons(include_arg)
    n_each = int(math.ceil(n_todo / ncore))
    core = (np.arange(n_todo) // n_each + 1).astype(np.int32)  # rep(seq(1, ncore), each = n_each)
    return pi, pj, core


# --------------------------------------------------------------------------------------------------
# sharding over ranks: the reference's `core` chunks (R/kendalltau.R:250-255) become GPU ranks
# --------------------------------------------------------------------------------------------------
def _dist_info():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist, dist.get_rank(), dist.get_world_size()
    except Exception:
        pass
    return None, 0, 1


def _run_sharded(engine, X, pi, pj, core, perspective, alternative, continuity):
    """Each rank computes the pairs whose `core` is rank+1, then all ranks gather everything.

    The HIP engine runs the whole sharded flow on the device (icikendalltau_amd/sharding.py): a rank uploads and
    sorts only its share of the columns, `order` + `meta` are all-gathered, the pair block runs, and the padded
    result blocks are all-gathered -- every buffer on the ENGINE's device (LOCAL_RANK-derived), never on torch's
    ambient current device.  Any other engine (the checker of the CPU tests) computes its block through
    engine.pairs() and the same gather.
    """
    dist, rank, world = _dist_info()
    if world == 1:
        return engine.pairs(X, pi, pj, perspective, alternative, continuity)
    import torch
    from . import sharding
    begin, end, n_each = sharding.pair_block(len(pi), rank, world)
    assert np.array_equal(np.nonzero(core == rank + 1)[0], np.arange(begin, end)), "core chunks are consecutive blocks"
    via_host = dist.get_backend() != "nccl"
    if hasattr(engine, "pairs_block_dev"):
        device = torch.device("cuda", engine.ctx.device)
        out_l, rsn_l = engine.pairs_block_dev(X, pi, pj, begin, end, n_each, perspective, alternative, continuity,
                                              dist, device, via_host)
    else:
        device = torch.device("cpu")
        out_l = torch.full((n_each, 4), float("nan"), dtype=torch.float64)
        rsn_l = torch.zeros(n_each, dtype=torch.int32)
        if end > begin:
            o, r = engine.pairs(X, pi[begin:end], pj[begin:end], perspective, alternative, continuity)
            out_l[:end - begin] = torch.from_numpy(np.ascontiguousarray(o))
            rsn_l[:end - begin] = torch.from_numpy(np.ascontiguousarray(r, dtype=np.int32))
    g_out = sharding.gather_blocks(dist, out_l, n_each, device, via_host or device.type == "cpu", to_all=True)
    g_rsn = sharding.gather_blocks(dist, rsn_l, n_each, device, via_host or device.type == "cpu", to_all=True)
    out = sharding.assemble(g_out, len(pi), n_each).cpu().numpy()
    rsn = sharding.assemble(g_rsn, len(pi), n_each).cpu().numpy()
    return out, rsn


# --------------------------------------------------------------------------------------------------
# ici_kendalltau (R/kendalltau.R:96-179) + scale_and_reshape (:357-421)
# --------------------------------------------------------------------------------------------------
def _host_masks(global_na) -> bool:
    """More distinct finite values than the device-side exclusion rule holds (MASK_VALS; the reference loops over any
    number, R/utils.R:16-20): the host has to mask the matrix."""
    vals = np.atleast_1d(np.asarray([] if global_na is None else global_na, dtype=np.float64))
    return len({float(v) for v in vals if math.isfinite(v)}) > _lib.MASK_VALS


def _mask_on_host(X, global_na):
    """(X, global_na) as a device entry takes them: unchanged, or -- _host_masks -- X masked here and NaN passed."""
    if not _host_masks(global_na):
        return X, global_na
    if _lib.is_sparse(X):
        X = _densify(X)
    X = np.asarray(X, dtype=np.float64)
    return _masked_fortran(X, setup_missing_matrix(X, global_na)), (float("nan"),)


def _warn_pairs(rcounts):
    """One warning per offending pair, as ici_split raises them."""
    for code in (_lib.REASON_SHORT, _lib.REASON_SINGLE_UNIQUE, _lib.REASON_TIES_EQ_TOTAL):
        for _ in range(int(rcounts[code])):
            _warn_reason(code)


def _max_taumax(taumax, where):
    """The largest taumax over the pairs `where` selects of a full result (-inf without one that is not NA)."""
    have = _na_rm(np.asarray(taumax)[where])
    return float(have.max()) if have.size else -math.inf


# -- what the selection entries (ici_kendalltau_topk ... ici_kendalltau_anosim below) share ----------------------
_TOPK_KEYS = ("cor", "raw", "pvalue", "taumax", "completeness")
_NA_REAL_BITS = np.uint64(0x7FF00000000007A2)   # R's NA_real_: what the library pads with


def _select_input(data_matrix, colnames):
    """The matrix of a selection entry after the input checks, read where it lies: (matrix, names, n_sample)."""
    data_matrix, names = _as_matrix(data_matrix, colnames, "data_matrix", keep_dtype=True, keep_sparse=True)
    return data_matrix, names, data_matrix.shape[1]


def _int_arg(value, lo, hi, message):
    """An integer in lo .. hi that is no bool, as an int; anything else is refused with `message`."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(message)
    return int(value)


def _timed(call):
    """The engine call(s) of a selection entry, timed together, and the warnings of their pairs: (the last call's result
    without its reason_counts, seconds)."""
    t1 = time.perf_counter()
    *out, rcounts = call()
    t_diff = time.perf_counter() - t1
    _warn_pairs(rcounts)
    return out, t_diff


def _on_device(eng, data_matrix, global_na, call):
    """_timed(call(X, global_na)) with the matrix and global_na as the engine's selection methods take them: masked on
    the host when the list is longer than the device rule, otherwise the caller's matrix where it lies."""
    X, global_na = _mask_on_host(data_matrix, global_na)
    X = _for_engine(X, eng, fortran=False)
    return _timed(lambda: call(X, global_na))


def _from_full(eng, data_matrix, names, global_na, perspective, scale_max, alternative, continuity, include_only=None,
               where=None):
    """The numpy route of an engine without the entry's method (the CPU tests' checker engines): ici_kendalltau on the
    whole matrix.  Returns (the five S x S planes in _TOPK_KEYS' order, run_time, max_taumax over the pairs `where`
    selects: the upper triangle unless given)."""
    full = ici_kendalltau(data_matrix, global_na=global_na, perspective=perspective, scale_max=scale_max, diag_good=True,
                          include_only=include_only, alternative=alternative, continuity=continuity, colnames=names,
                          engine=eng)
    if where is None:
        where = np.triu_indices(len(names), k=1)
    return [np.asarray(full[key]) for key in _TOPK_KEYS], full["run_time"], _max_taumax(full["taumax"], where)


def _na_filled(shape):
    """A float64 array filled with R's NA_real_."""
    a = np.empty(shape, dtype=np.float64)
    a.view(np.uint64)[...] = _NA_REAL_BITS
    return a


def _put_values(res, vals5, prefix=""):
    """The five value columns of a selection into the result dict."""
    for q, key in enumerate(_TOPK_KEYS):
        res[prefix + key] = vals5[q]


def _named_matrix(values: np.ndarray, names):
    if pd is not None:
        return pd.DataFrame(values, index=list(names), columns=list(names))
    return values


def ici_kendalltau(data_matrix, global_na=(float("nan"), float("inf"), 0), perspective="global", scale_max=True,
                   diag_good=True, include_only=None, alternative="two.sided", continuity=False,
                   check_timing=False, return_matrix=True, colnames=None, engine=None, n_gpu=1, devices=None):
    """All-pairs ICI-Kendall-tau between the COLUMNS (samples) of a features x samples matrix.

    ``n_gpu`` > 1 (or ``devices``) uses several MI355X behind one library call (icikt_pairs_multi_f64: a host
    thread per GPU, RCCL all-gather / gather over xGMI) -- the role furrr workers play in the reference
    (R/kendalltau.R:127,158): the `core` column then numbers the GPUs' pair blocks.  Under an initialised
    torch.distributed process group the ranks are the cores instead (one process per GPU).

    Mirrors R/kendalltau.R:96-179: same argument names and defaults; returns a dict with ``cor, raw,
    pvalue, taumax, completeness`` (samples x samples, un-computed cells 0), ``keep`` and ``run_time``,
    or with ``return_matrix=False`` ``{"cor": data.frame(s1, s2, core, raw, pvalue, taumax,
    completeness, cor), "run_time"}``.  Column names are required, as in the reference (``colnames=``
    for a bare ndarray).

    ``data_matrix`` may be a sparse matrix (scipy.sparse of any format, features x samples; column names from
    ``colnames=``): with the default ``global_na`` its absent cells are the missing ones.  On one MI355X its CSC arrays
    go to the device as they are (icikt_matrix_csc; other formats through ``tocsc()``, O(nnz)).  The branches that edit
    the matrix on the host densify it with ``toarray()``: ``check_timing``, ``return_matrix=False``, more than 32
    finite ``global_na`` values, several GPUs or ranks, and an ``engine`` that is not the HIP one.
    """
    data_matrix, names = _as_matrix(data_matrix, colnames, "data_matrix", keep_dtype=True, keep_sparse=True)
    n_sample = data_matrix.shape[1]

    _dist, _rank, world = _dist_info()
    ncore = world
    if engine is None and world == 1 and (n_gpu > 1 or devices is not None):
        engine = _multi_engine(n_gpu, devices)
        ncore = len(engine.ctx.devices)
    eng = engine or _default_engine()

    host_masks = _host_masks(global_na)   # a list longer than the device-side rule takes the host-masking route below
    if return_matrix and not check_timing and world == 1 and hasattr(eng, "matrix") and not host_masks:
        # One library call does everything below the argument checks on the device (icikt_matrix_f64): the exclusion
        # rule of setup_missing_matrix inside the pre-pass (no masked copy of the matrix on the host), the pair
        # kernels, scale_and_reshape, one copy of the five matrices back.  All pairs of the upper triangle need no
        # pair list at all; include_only / diag_good = FALSE hand over the filtered list.
        if include_only is None and diag_good:
            _need_pairs(n_sample)
            pi = pj = None
        else:
            pi, pj, _core = setup_comparisons(names, include_only, diag_good, ncore=ncore)
        t1 = time.perf_counter()
        out5, keep, rcounts = eng.matrix(_for_engine(data_matrix, eng, fortran=False), global_na, pi, pj, perspective, alternative, continuity,
                                         scale_max, diag_good)
        t_diff = time.perf_counter() - t1
        _warn_pairs(rcounts)
        res = {key: _named_matrix(out5[k], names)
               for k, key in enumerate(("cor", "raw", "pvalue", "taumax", "completeness"))}
        res["keep"] = keep
        res["run_time"] = t_diff
        return res

    if _lib.is_sparse(data_matrix):
        data_matrix = _densify(data_matrix)
    data_matrix = np.asarray(data_matrix, dtype=np.float64)   # (the branches below edit the matrix on the host)
    exclude_loc = setup_missing_matrix(data_matrix, global_na)
    exclude_data = _masked_fortran(data_matrix, exclude_loc)
    pi, pj, core = setup_comparisons(names, include_only, diag_good, ncore=ncore)
    n_todo = len(pi)

    if check_timing:  # R/kendalltau.R:141-148, 633-669
        rng = np.random.default_rng()
        first = np.nonzero(core == 1)[0]
        pick = rng.choice(first, size=min(5, len(first)), replace=False)
        t0 = time.perf_counter()
        for p in pick:
            eng.pairs(exclude_data, pi[p:p + 1], pj[p:p + 1], perspective, "two.sided", False)
        t_total = time.perf_counter() - t0
        n_comp = len(pick)
        t_each = t_total / n_comp
        t_theoretical = t_each * n_todo
        t_cores = t_theoretical / ncore
        which = ["n_tested", "n_todo", "time_tested", "time_single", "time_all", "time_across_cores",
                 "time_minutes", "time_hours", "time_days"]
        value = [n_comp, n_todo, t_total, t_each, t_theoretical, t_cores, t_cores / 60, t_cores / (60 * 60),
                 t_cores / (60 * 60 * 60)]  # (sic) the reference divides by 60^3 for days
        return pd.DataFrame({"which": which, "value": value}) if pd is not None else dict(zip(which, value))

    t1 = time.perf_counter()
    out, rsn = _run_sharded(eng, exclude_data, pi, pj, core, perspective, alternative, continuity)
    t_diff = time.perf_counter() - t1
    for r in rsn[rsn > 1]:
        _warn_reason(r)

    raw, pvalue, taumax, completeness = out[:, 0], out[:, 1], out[:, 2], out[:, 3]
    n_good = (exclude_loc.shape[0] - exclude_loc.sum(axis=0)).astype(np.float64)
    frac_complete = n_good / exclude_loc.shape[0]

    # scale_and_reshape
    if scale_max:
        have = _na_rm(taumax)                                           # max(taumax, na.rm = TRUE)
        max_cor = have.max() if have.size else -np.inf                  # max(numeric(0)) is -Inf in R (and in k_assemble)
        cor = raw / max_cor
    else:
        cor = raw.copy()
    s1, s2 = pi.copy(), pj.copy()
    core_col = core.astype(np.float64)
    if diag_good:
        d = np.arange(n_sample, dtype=np.int32)
        s1 = np.concatenate([s1, d])
        s2 = np.concatenate([s2, d])
        core_col = np.concatenate([core_col, np.zeros(n_sample)])
        diag = n_good / n_good.max()
        raw = np.concatenate([raw, diag])
        pvalue = np.concatenate([pvalue, np.zeros(n_sample)])
        taumax = np.concatenate([taumax, np.ones(n_sample)])
        completeness = np.concatenate([completeness, frac_complete])
        cor = np.concatenate([cor, diag])

    if return_matrix:
        res = {}
        for key, vals in (("cor", cor), ("raw", raw), ("pvalue", pvalue), ("taumax", taumax),
                          ("completeness", completeness)):
            m = np.zeros((n_sample, n_sample))
            m[s1, s2] = vals
            m[s2, s1] = vals
            res[key] = _named_matrix(m, names)
        res["keep"] = (~exclude_loc).T
        res["run_time"] = t_diff
        return res
    names_arr = np.asarray(names, dtype=object)
    cols = {"s1": names_arr[s1], "s2": names_arr[s2], "core": core_col, "raw": raw, "pvalue": pvalue,
            "taumax": taumax, "completeness": completeness, "cor": cor}
    return {"cor": pd.DataFrame(cols) if pd is not None else cols, "run_time": t_diff}


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_topk: every sample's k nearest partners (no counterpart in the reference)
# --------------------------------------------------------------------------------------------------
def _best_per_row(mats5, k, skip_own):
    """Per row of five matrices (cor, raw, pvalue, taumax, completeness) the k columns whose raw is not NA -- without the
    row's own index when skip_own --, by raw descending in the order of the doubles' bits (-0.0 below +0.0), ties by the
    smaller index; padding -1 / NA_real_.  Returns (idx [rows, k], vals5 [5, rows, k], n_valid [rows])."""
    mats5 = [np.ascontiguousarray(m, dtype=np.float64) for m in mats5]
    raw = mats5[1]
    n_rows, n_cols = raw.shape
    idx = np.full((n_rows, k), -1, dtype=np.int32)
    vals = _na_filled((5, n_rows, k))
    n_valid = np.zeros(n_rows, dtype=np.int32)
    bits = raw.view(np.uint64)
    sign = (bits >> np.uint64(63)).astype(bool)
    key = np.where(sign, ~bits, bits | np.uint64(1 << 63))
    cols = np.arange(n_cols)
    for r in range(n_rows):
        ok = ~np.isnan(raw[r])
        if skip_own:
            ok[r] = False
        cand = cols[ok]
        sel = cand[np.lexsort((cand, ~key[r, cand]))[:k]]     # ~key ascending = key descending, then the index
        m = len(sel)
        n_valid[r] = m
        idx[r, :m] = sel
        for q in range(5):
            vals[q, r, :m] = mats5[q][r, sel]
    return idx, vals, n_valid


def _topk_numpy(mats5, k):
    """The selection of icikt_topk_f64 from five full S x S matrices (cor, raw, pvalue, taumax, completeness), for
    engines without a topk method (the CPU tests' checker engines).  Per column: partners j != c whose raw is not NA,
    by raw descending in the order of the doubles' bits (-0.0 below +0.0), ties by the smaller index; padding -1 /
    NA_real_.  Returns (idx [S, k], vals5 [5, S, k], n_valid [S])."""
    return _best_per_row(mats5, k, skip_own=True)


def ici_kendalltau_topk(data_matrix, k, global_na=(float("nan"), float("inf"), 0), perspective="global", scale_max=True,
                        alternative="two.sided", continuity=False, colnames=None, engine=None):
    """For every sample (column) of a features x samples matrix its ``k`` partners with the largest ICI-Kendall-tau:
    the rows of a kNN graph, without the S x S matrices ``ici_kendalltau`` returns.

    The arguments are ``ici_kendalltau``'s (column names are required; a sparse matrix, float32 and integer matrices
    are read where they lie).  On the HIP engine the selection runs on the device (icikt_topk_f64) and nothing of size
    S x S exists on either side; ``k`` is an integer in 1 .. 256, and a matrix has at most 65 535 samples.

    Partners are ordered by ``raw`` descending, ties by the smaller sample index; a pair whose ``raw`` is NA is no
    one's partner (the reference's warning is raised once per such pair of reasons 2-4); ``cor`` is ``raw`` over the
    largest ``taumax`` of all pairs when ``scale_max``.  Returns a dict: ``indices`` (S x k, -1 where a sample has fewer
    than k partners), ``neighbors`` (their names, None padded), ``cor, raw, pvalue, taumax, completeness`` (S x k, NA
    padded), ``n_valid`` (S), ``max_taumax`` and ``run_time``.  ``formats.topk_to_csr`` turns it into a sparse graph.
    """
    k = _int_arg(k, 1, _lib.TOPK_MAX, f"`k` must be an integer in 1 .. {_lib.TOPK_MAX}")
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    _need_pairs(n_sample)
    eng = engine or _default_engine()
    if hasattr(eng, "topk"):
        (idx, vals, n_valid, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.topk(X, k, gna, perspective, alternative, continuity, 0, scale_max))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, scale_max, alternative,
                                               continuity)
        idx, vals, n_valid = _topk_numpy(mats5, k)
    names_arr = np.asarray(list(names) + [None], dtype=object)
    res = {"indices": idx, "neighbors": names_arr[idx]}    # (-1 picks the None behind the names)
    _put_values(res, vals)
    res["n_valid"] = n_valid
    res["max_taumax"] = max_taumax
    res["run_time"] = t_diff
    return res


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_cross: query samples against a reference cohort (R's cor(x, y) for ICI-Kt; no counterpart in the
# reference)
# --------------------------------------------------------------------------------------------------
def _cross_topk_numpy(mats5, k):
    """The selection of icikt_cross_f64 from five Sq x Sr matrices (cor, raw, pvalue, taumax, completeness): per query
    row the reference columns whose raw is not NA, by raw descending in the order of the doubles' bits (-0.0 below
    +0.0), ties by the smaller index; padding -1 / NA_real_.  Returns (idx [Sq, k], vals5 [5, Sq, k], n_valid [Sq])."""
    return _best_per_row(mats5, k, skip_own=False)


def _cross_numpy(eng, query, reference, global_na, perspective, scale_max, alternative, continuity):
    """The rectangle on an engine without a cross method (the CPU tests' checker engines): ``ici_kendalltau`` on the
    stacked matrix with ``include_only`` = the rectangle's pairs -- so ``cor`` is scaled by the rectangle's largest
    taumax -- and the [query, reference] block of its matrices.  Returns (mats5 [5, Sq, Sr], max_taumax, run_time)."""
    Sq, Sr = query.shape[1], reference.shape[1]
    if Sq == 0 or Sr == 0:
        return np.empty((5, Sq, Sr)), -math.inf, 0.0
    stacked = np.hstack([np.asarray(query, dtype=np.float64), np.asarray(reference, dtype=np.float64)])
    qn, rn = [f"q{i}" for i in range(Sq)], [f"r{j}" for j in range(Sr)]     # (the callers' names may repeat across the two)
    block = (slice(0, Sq), slice(Sq, None))
    mats5, run_time, max_taumax = _from_full(eng, stacked, qn + rn, global_na, perspective, scale_max, alternative,
                                             continuity, include_only=[list(np.repeat(qn, Sr)), rn * Sq], where=block)
    return np.stack([m[block] for m in mats5]), max_taumax, run_time


def _cross_class_numpy(cor, raw, cls, n_class):
    """The class reduction of icikt_ref_cross_f64 from the Sq x Sr cor and raw matrices of a rectangle, for engines
    without a prepared reference (the CPU tests' checker engines).  The partners of cell (q, c) are the reference
    columns r with cls[r] == c whose raw with q is not NA -- there is no own sample on a rectangle; the medians are
    _median_cell's.  Returns (med2 [2, Sq, n_class]: cor, raw; n_valid [Sq, n_class])."""
    cor = np.ascontiguousarray(cor, dtype=np.float64)
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    cls = np.asarray(cls)
    Sq = raw.shape[0]
    med2 = _na_filled((2, Sq, n_class))
    n_valid = np.zeros((Sq, n_class), dtype=np.int32)
    members = [cls == c for c in range(n_class)]
    for q in range(Sq):
        valid = ~np.isnan(raw[q])
        for c in range(n_class):
            partners = np.nonzero(members[c] & valid)[0]
            n_valid[q, c] = len(partners)
            if len(partners):
                med2[0, q, c], med2[1, q, c] = _median_cell(cor, raw, q, partners)
    return med2, n_valid


def _global_na_rule(global_na):
    """What a global_na list excludes, whatever its order or repeats: (NA, Inf, the finite values)."""
    vals = [float(v) for v in np.atleast_1d(np.asarray([] if global_na is None else global_na, dtype=np.float64))]
    return (any(math.isnan(v) for v in vals), any(math.isinf(v) for v in vals),
            frozenset(v for v in vals if math.isfinite(v)))


_CROSS_GLOBAL_NA = (float("nan"), float("inf"), 0)   # ici_kendalltau_cross' default, told from a caller's value by identity


class PreparedReference:
    """A reference cohort kept ready for batch after batch of ``ici_kendalltau_cross`` (``prepare_reference`` makes it).

    On the HIP engine the reference is uploaded and pre-passed once and stays on the device, on a context of its own, so
    no other call can displace it; ``close()`` (or leaving a ``with`` block) frees it.  On an engine without a prepared
    reference (the CPU tests' checker engines) it holds the host matrix and every batch takes the numpy route.  It
    carries what a batch needs beside its own columns: ``reference_names``, ``global_na``, ``class_levels`` and
    ``class_codes`` (None without classes), ``n_feat``, ``n_reference`` and ``query_capacity``."""

    def __init__(self, engine, reference, names, query_capacity, global_na, levels, codes):
        self.engine = engine
        self.reference_names = list(names)
        self.n_feat, self.n_reference = reference.shape
        self.query_capacity = int(query_capacity)
        self.global_na = global_na
        self.class_levels = None if levels is None else list(levels)
        self.class_codes = codes
        self._matrix = self._ctx = None
        if hasattr(engine, "prepare_reference"):
            masked, self._device_na = _mask_on_host(reference, global_na)
            self._ctx = engine.prepare_reference(masked, self.query_capacity, self._device_na)
        else:
            self._matrix = np.asarray(reference, dtype=np.float64)

    def close(self):
        """Free the device copy (a closed reference takes no more batches)."""
        if self._ctx is not None:
            self._ctx.close()
        self._ctx = self._matrix = None
        self.engine = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _batch(self, query, k, want_matrix, want_classes, perspective, scale_max, alternative, continuity):
        """One batch of at most query_capacity columns: (out5, idx, vals, n_valid, max_taumax, med2, cls_n_valid, seconds),
        the tables as Context.cross_prepared returns them."""
        if self.engine is None:
            raise ValueError("this PreparedReference has been closed")
        n_class = len(self.class_levels) if want_classes else 0
        if self._ctx is not None:
            query, _ = _mask_on_host(query, self.global_na)
            (out5, idx, vals, n_valid, max_taumax, med2, cls_n_valid), t_diff = _timed(
                lambda: _rcounts_last(self._ctx.cross_prepared(
                    query, k, want_matrix, self.class_codes if want_classes else None, n_class, perspective, alternative,
                    continuity, getattr(self.engine, "flags", 0), scale_max)))
            return out5, idx, vals, n_valid, max_taumax, med2, cls_n_valid, t_diff
        out5, max_taumax, t_diff = _cross_numpy(self.engine, query, self._matrix, self.global_na, perspective, scale_max,
                                                alternative, continuity)
        idx = vals = n_valid = med2 = cls_n_valid = None
        if k is not None:
            idx, vals, n_valid = _cross_topk_numpy(out5, k)
        if want_classes:
            med2, cls_n_valid = _cross_class_numpy(out5[0], out5[1], self.class_codes, n_class)
        return out5 if want_matrix else None, idx, vals, n_valid, max_taumax, med2, cls_n_valid, t_diff


def _rcounts_last(items):
    """Context.cross_prepared's tuple with reason_counts moved to the end, where _timed takes it from."""
    out5, idx, vals, n_valid, max_taumax, rcounts, med2, cls_n_valid = items
    return out5, idx, vals, n_valid, max_taumax, med2, cls_n_valid, rcounts


def prepare_reference(reference, query_capacity=1024, global_na=(float("nan"), float("inf"), 0), reference_names=None,
                      reference_classes=None, engine=None):
    """Keep ``reference`` (features x Sr) ready for ``ici_kendalltau_cross``: on the HIP engine it is uploaded and
    pre-passed here, once, and every later batch brings its own columns alone (icikt_ref_prepare_f64).

    ``query_capacity`` (an integer of at least 1) is the widest batch the device copy takes in one call; its memory is
    allocated here and never grows, and a wider batch is split by ``ici_kendalltau_cross``.  Sr + query_capacity is at
    most 65 535 (one less for each of the two that is odd).  ``global_na`` is recorded and applies to every batch.
    ``reference_names`` as ``ici_kendalltau_cross`` takes them; ``reference_classes`` gives one label per reference
    column and makes every batch return the class tables.  Returns a ``PreparedReference``; close it, or use it in a
    ``with`` block, to free the device memory."""
    query_capacity = _int_arg(query_capacity, 1, _lib.TOPK_MAX_SAMPLES,
                              f"`query_capacity` must be an integer in 1 .. {_lib.TOPK_MAX_SAMPLES}")
    reference, rnames = _as_matrix(reference, reference_names, "reference", keep_dtype=True)
    levels = codes = None
    if reference_classes is not None:
        try:
            levels, codes = _class_levels(reference_classes, reference.shape[1], "all")
        except ValueError:
            raise ValueError("`reference_classes` must give one class per column of `reference`") from None
    return PreparedReference(engine or _default_engine(), reference, rnames, query_capacity, global_na, levels, codes)


def _cross_prepared(query, prepared, k, return_matrix, perspective, scale_max, alternative, continuity):
    """ici_kendalltau_cross against a PreparedReference: the batch in capacity-sized parts, stitched."""
    Sq, cap = query.shape[1], prepared.query_capacity
    classes = prepared.class_levels is not None
    parts = [prepared._batch(query[:, a:a + cap], k, return_matrix, classes, perspective, scale_max, alternative, continuity)
             for a in range(0, max(Sq, 1), cap)]
    widths = [min(cap, Sq - a) for a in range(0, max(Sq, 1), cap)]
    max_taumax = max(p[4] for p in parts)
    t_diff = sum(p[7] for p in parts)

    def stitch(item, axis):
        return parts[0][item] if len(parts) == 1 else np.concatenate([p[item] for p in parts], axis=axis)

    out5 = stitch(0, 1) if return_matrix else None
    idx, vals, n_valid = (stitch(1, 0), stitch(2, 1), stitch(3, 0)) if k is not None else (None, None, None)
    med2, cls_n_valid = (stitch(5, 1), stitch(6, 0)) if classes else (None, None)
    if scale_max and len(parts) > 1:
        # every part scaled cor by ITS largest taumax: the parts below the call's are scaled again, from raw
        a = 0
        for p, w in zip(parts, widths):
            if p[4] != max_taumax:
                rows = slice(a, a + w)
                for planes in (out5, vals):
                    if planes is not None:
                        ok = ~np.isnan(planes[1][rows])
                        planes[0][rows][ok] = planes[1][rows][ok] / max_taumax
                if classes:   # an odd cell's median is one pair's cor; an even cell's two quotients are not kept:
                    # its median is reduced again, on the host, from the part's raw (asked for if the call kept none)
                    odd, even = (cls_n_valid[rows] & 1) == 1, (cls_n_valid[rows] > 0) & ((cls_n_valid[rows] & 1) == 0)
                    med2[0][rows][odd] = med2[1][rows][odd] / max_taumax + 0.0
                    if even.any():
                        part5 = p[0]
                        if part5 is None:   # (its pairs were warned about the first time; the five planes of this
                            with warnings.catch_warnings():   # one part exist only until its even cells are reduced)
                                warnings.simplefilter("ignore")
                                again = prepared._batch(query[:, a:a + w], None, True, False, perspective, False,
                                                        alternative, continuity)
                            part5, t_diff = again[0], t_diff + again[7]
                        part_raw = np.ascontiguousarray(part5[1], dtype=np.float64)
                        part_cor, ok = np.full(part_raw.shape, np.nan), ~np.isnan(part_raw)
                        part_cor[ok] = part_raw[ok] / max_taumax
                        host = _cross_class_numpy(part_cor, part_raw, prepared.class_codes,
                                                  len(prepared.class_levels))[0]
                        med2[0][rows][even] = host[0][even]
            a += w
    return out5, idx, vals, n_valid, max_taumax, med2, cls_n_valid, t_diff


def ici_kendalltau_cross(query, reference, k=None, return_matrix=True, global_na=_CROSS_GLOBAL_NA,
                         perspective="global", scale_max=True, alternative="two.sided", continuity=False,
                         query_names=None, reference_names=None, reference_classes=None, engine=None):
    """ICI-Kendall-tau of every sample (column) of ``query`` with every sample of ``reference`` -- a new batch against
    a reference cohort -- and nothing else: no pair within either matrix is computed.

    ``query`` (features x Sq) and ``reference`` (features x Sr) share their rows; column names are required for both
    (``query_names=`` / ``reference_names=`` for bare ndarrays).  ``global_na``, ``perspective``, ``alternative`` and
    ``continuity`` are ``ici_kendalltau``'s and apply to both matrices.  float32 and integer matrices of either memory
    order are read where they lie; a sparse matrix is densified on the host (``toarray()``).  On the HIP engine the
    rectangle runs on the device (icikt_cross_f64); Sq + Sr is at most 65 535 (one less when Sq is odd).

    ``cor`` is ``raw`` over the largest ``taumax`` of the rectangle's pairs when ``scale_max`` -- what
    ``ici_kendalltau(include_only=<those pairs>)`` scales by -- else ``raw``.  With ``k`` (an integer in 1 .. 256) every
    query gets its ``k`` reference samples with the largest ``raw``: ``raw`` descending, ties by the smaller reference
    index; a pair whose ``raw`` is NA is no partner.  A sample that occurs in both matrices is a partner like any other
    (it is usually its own nearest reference sample).  The reference's warning is raised once per pair of reasons 2-4.

    ``reference`` may be a ``PreparedReference`` (``prepare_reference``): the names, ``global_na`` and the classes are
    then its own -- ``reference_names`` and ``reference_classes`` are refused, and so is a ``global_na`` that differs
    from the one it was prepared with -- and only the batch crosses to the device.  A batch wider than its
    ``query_capacity`` is split into capacity-sized calls and stitched; with ``scale_max`` ``cor`` is then scaled again,
    from ``raw``, by the largest ``max_taumax`` of the parts, and ``class_med_cor`` likewise (an even cell's median is
    reduced again on the host from the part's ``raw``), so a split call gives an unsplit call's bits.  Everything derived
    from ``raw`` alone -- ``raw``, ``pvalue``, ``taumax``, ``completeness``, the top-k selection, ``class_med_raw``,
    ``class_n_valid``, ``nearest_class`` -- does not depend on the split.

    ``reference_classes`` (one label per reference column; with a plain matrix the reference is prepared for this one
    call) adds every query's median to every class: the partners of cell (q, c) are the reference samples of class c
    whose pair with q has a ``raw`` that is not NA, ``class_med_raw`` is R's ``median(raw, na.rm = TRUE)`` over them and
    ``class_med_cor`` the same over ``cor``; a cell without a partner is NA.

    Returns a dict.  With ``return_matrix``: ``cor, raw, pvalue, taumax, completeness`` as Sq x Sr tables, rows the
    query samples.  With ``k``: ``indices`` (Sq x k reference column indices, -1 where a query has fewer than k
    partners), ``neighbors`` (their names, None padded), ``topk_cor, topk_raw, topk_pvalue, topk_taumax,
    topk_completeness`` (Sq x k, NA padded) and ``n_valid`` (Sq); ``formats.cross_topk_to_csr`` turns them into a
    sparse graph.  With classes: ``class_med_cor``, ``class_med_raw`` and ``class_n_valid`` (Sq x C tables, the class
    levels as columns), ``class_levels`` and ``nearest_class`` (per query the label of the class with the largest
    ``class_med_raw`` among the cells with a partner, ties to the earlier class, None without one).  Always:
    ``query_names``, ``reference_names``, ``max_taumax`` and ``run_time``.  An empty ``query`` or ``reference`` gives
    empty tables.
    """
    if k is not None:
        k = _int_arg(k, 1, _lib.TOPK_MAX, f"`k` must be None or an integer in 1 .. {_lib.TOPK_MAX}")
    elif not return_matrix and reference_classes is None and not (isinstance(reference, PreparedReference)
                                                                  and reference.class_levels is not None):
        raise ValueError("nothing to return: give `k`, or leave `return_matrix` set")
    query, qnames = _as_matrix(query, query_names, "query", keep_dtype=True)
    prepared = reference if isinstance(reference, PreparedReference) else None
    eng = engine or (prepared.engine if prepared is not None else _default_engine())
    out5 = idx = vals = n_valid = med2 = cls_n_valid = None
    if prepared is not None:
        if reference_names is not None or reference_classes is not None:
            raise ValueError("`reference_names` and `reference_classes` belong to the PreparedReference: give them to "
                             "prepare_reference")
        if global_na is not _CROSS_GLOBAL_NA and _global_na_rule(global_na) != _global_na_rule(prepared.global_na):
            raise ValueError("`global_na` differs from the one the PreparedReference was prepared with")
        if engine is not None and engine is not prepared.engine:
            raise ValueError("`engine` differs from the PreparedReference's")
    else:
        reference, rnames = _as_matrix(reference, reference_names, "reference", keep_dtype=True)
    n_ref_rows = prepared.n_feat if prepared is not None else reference.shape[0]
    if query.shape[0] != n_ref_rows:
        raise ValueError(f"`query` has {query.shape[0]} rows (features) and `reference` has {n_ref_rows}: "
                         "the two must share their rows")
    Sq = query.shape[1]
    if prepared is None and reference_classes is not None:
        # a labelled plain matrix: prepared for this one call, with room for the whole batch
        Sr = reference.shape[1]
        room = _lib.TOPK_MAX_SAMPLES - Sr - (Sr & 1)
        cap = max(1, min(Sq, room - (room & 1)))
        with prepare_reference(reference, cap, global_na, rnames, reference_classes, eng) as temp:
            return ici_kendalltau_cross(query, temp, k, return_matrix, perspective=perspective, scale_max=scale_max,
                                        alternative=alternative, continuity=continuity, query_names=qnames, engine=eng)
    if prepared is not None:
        rnames = prepared.reference_names
        out5, idx, vals, n_valid, max_taumax, med2, cls_n_valid, t_diff = _cross_prepared(
            query, prepared, k, return_matrix, perspective, scale_max, alternative, continuity)
    elif hasattr(eng, "cross"):   # (two matrices, handed over as they are: the parts of _on_device that fit)
        query, _ = _mask_on_host(query, global_na)
        reference, global_na = _mask_on_host(reference, global_na)
        (out5, idx, vals, n_valid, max_taumax), t_diff = _timed(
            lambda: eng.cross(query, reference, k, return_matrix, global_na, perspective, alternative, continuity, 0,
                              scale_max))
    else:
        out5, max_taumax, t_diff = _cross_numpy(eng, query, reference, global_na, perspective, scale_max, alternative,
                                                continuity)
        if k is not None:
            idx, vals, n_valid = _cross_topk_numpy(out5, k)
    res = {}
    if return_matrix:
        for f, key in enumerate(_TOPK_KEYS):
            res[key] = pd.DataFrame(out5[f], index=list(qnames), columns=list(rnames)) if pd is not None else out5[f]
    if k is not None:
        names_arr = np.asarray(list(rnames) + [None], dtype=object)
        res["indices"] = idx
        res["neighbors"] = names_arr[idx]    # (-1 picks the None behind the names)
        _put_values(res, vals, "topk_")
        res["n_valid"] = n_valid
    if med2 is not None:
        levels = prepared.class_levels

        def table(values):
            return pd.DataFrame(values, index=list(qnames), columns=list(levels)) if pd is not None else values
        res["class_med_cor"] = table(med2[0])
        res["class_med_raw"] = table(med2[1])
        res["class_n_valid"] = table(cls_n_valid)
        res["class_levels"] = list(levels)
        res["nearest_class"] = _nearest_class(med2[1], cls_n_valid, levels)
    res["query_names"] = list(qnames)
    res["reference_names"] = list(rnames)
    res["max_taumax"] = max_taumax
    res["run_time"] = t_diff
    return res


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_medians: every sample's median ICI-Kendall-tau over the other samples of its class (the outlier
# screen the matrix is computed for; the reference leaves the reduction to the user)
# --------------------------------------------------------------------------------------------------
def _r_median_pair(a, b):
    """R's mean() of the two middle values, a zero as +0 (the even branch of _r_median_sorted)."""
    s = a + b
    if math.isfinite(s):
        return 0.5 * s + 0.0
    if math.isfinite(a) and math.isfinite(b):
        return 0.5 * a + 0.5 * b + 0.0
    return float(np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]) if math.isnan(s) else s


def _median_cell(cor, raw, s, partners):
    """(med_cor, med_raw) of sample s over its partners (at least one): the middle one of their raw values sorted
    ascending (a zero counts as +0), or R's mean of the two middle ones, and the same rule on the cor cells of the
    partners that supplied those raw values."""
    v = len(partners)
    order = np.argsort(raw[s, partners] + 0.0, kind="stable")
    mid = partners[order[[(v - 1) // 2, v // 2]]]       # (twice the same partner when v is odd)
    cell = []
    for mat in (cor, raw):
        a, b = float(mat[s, mid[0]]) + 0.0, float(mat[s, mid[1]]) + 0.0
        cell.append(a if v & 1 else _r_median_pair(a, b))
    return cell


def _class_medians_numpy(cor, raw, cls):
    """The reduction of icikt_class_medians_f64 from full S x S cor and raw matrices, for engines without a
    class_medians method (the CPU tests' checker engines).  The partners of sample s are the other samples of its class
    whose raw with s is not NA; n_valid[s] counts them.  med_raw[s] is R's median(raw, na.rm = TRUE) over them: with the
    values sorted ascending (a zero counts as +0), the middle one, or the mean of the two middle ones; med_cor[s] is
    the same rule on the cor cells of the partners that supplied those middle raw values.  Without partners both are
    NA_real_.  Returns (med2 [2, S]: cor, raw; n_valid [S])."""
    cor = np.ascontiguousarray(cor, dtype=np.float64)
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    cls = np.asarray(cls)
    S = raw.shape[0]
    med2 = _na_filled((2, S))
    n_valid = np.zeros(S, dtype=np.int32)
    for s in range(S):
        ok = (cls == cls[s]) & ~np.isnan(raw[s])
        ok[s] = False
        partners = np.nonzero(ok)[0]
        n_valid[s] = len(partners)
        if len(partners):
            med2[0, s], med2[1, s] = _median_cell(cor, raw, s, partners)
    return med2, n_valid


def ici_kendalltau_medians(data_matrix, sample_classes=None, global_na=(float("nan"), float("inf"), 0),
                           perspective="global", scale_max=True, alternative="two.sided", continuity=False,
                           colnames=None, engine=None):
    """For every sample (column) of a features x samples matrix the median ICI-Kendall-tau to the other samples of its
    class: the outlier screen of a quality-control run, without the S x S matrices ``ici_kendalltau`` returns and
    without computing a pair that crosses classes.

    ``sample_classes`` gives one label per column (None: one class); the other arguments are ``ici_kendalltau``'s
    (column names are required; a sparse matrix, float32 and integer matrices are read where they lie).  On the HIP
    engine the reduction runs on the device (icikt_class_medians_f64); a matrix has at most 65 535 samples.

    The partners of a sample are the other samples of its class whose pair with it has a ``raw`` that is not NA (the
    reference's warning is raised once per pair of reasons 2-4).  ``med_raw`` is R's ``median(raw, na.rm = TRUE)`` over
    them, and ``med_cor`` the same over ``cor``.  With ``scale_max`` ``cor`` is ``raw`` over the largest ``taumax`` of
    the COMPUTED, that is within-class, pairs -- what ``ici_kendalltau(include_only = <those pairs>)`` scales by, not
    the maximum over all S (S - 1) / 2 pairs; ``med_raw`` does not depend on it.  A sample without a partner (a
    singleton class among them) gets NA.  Returns a dict: ``sample_id`` and ``sample_class`` (names and labels in
    column order), ``med_cor``, ``med_raw``, ``n_valid`` (S each), ``max_taumax`` (-inf when no pair was computed) and
    ``run_time``.
    """
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    levels, cls = _class_levels(sample_classes, n_sample, "all")
    _need_pairs(n_sample)
    eng = engine or _default_engine()
    if hasattr(eng, "class_medians"):
        (med2, n_valid, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.class_medians(X, cls, len(levels), gna, perspective, alternative, continuity, 0, scale_max))
    else:
        # the within-class pairs, class by class, combn order inside a class
        first, second = [], []
        for k in range(len(levels)):
            members = np.nonzero(cls == k)[0]
            a, b = np.triu_indices(len(members), k=1)
            first.extend(names[i] for i in members[a])
            second.extend(names[i] for i in members[b])
        if first:
            same = (cls[:, None] == cls[None, :]) & np.triu(np.ones((n_sample, n_sample), dtype=bool), k=1)
            mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, scale_max,
                                                   alternative, continuity, include_only=[first, second], where=same)
            med2, n_valid = _class_medians_numpy(mats5[0], mats5[1], cls)
        else:   # singletons alone: nothing to compute
            t_diff, max_taumax = 0.0, -math.inf
            med2, n_valid = _na_filled((2, n_sample)), np.zeros(n_sample, dtype=np.int32)
    labels = [levels[k] for k in cls]
    return {"sample_id": list(names), "sample_class": labels, "med_cor": med2[0], "med_raw": med2[1],
            "n_valid": n_valid, "max_taumax": max_taumax, "run_time": t_diff}


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_class_matrix: every sample's median ICI-Kendall-tau to every class (the table a mislabelled or
# swapped sample shows up in, and from which an unlabelled one is assigned; the reference leaves it to the user)
# --------------------------------------------------------------------------------------------------
def _class_matrix_numpy(cor, raw, cls, n_class):
    """The reduction of icikt_class_matrix_f64 from full S x S cor and raw matrices, for engines without a class_matrix
    method (the CPU tests' checker engines).  The partners of cell (s, c) are the samples t != s with cls[t] == c whose
    raw with s is not NA; n_valid[s, c] counts them.  med_raw[s, c] is R's median(raw, na.rm = TRUE) over them
    (_class_medians_numpy's rule), med_cor[s, c] the same rule on the cor cells of the partners that supplied the middle
    raw values.  Without partners both are NA_real_.  Returns (med2 [2, S, n_class]: cor, raw; n_valid [S, n_class])."""
    cor = np.ascontiguousarray(cor, dtype=np.float64)
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    cls = np.asarray(cls)
    S = raw.shape[0]
    med2 = _na_filled((2, S, n_class))
    n_valid = np.zeros((S, n_class), dtype=np.int32)
    members = [cls == c for c in range(n_class)]
    for s in range(S):
        valid = ~np.isnan(raw[s])
        valid[s] = False
        for c in range(n_class):
            partners = np.nonzero(members[c] & valid)[0]
            n_valid[s, c] = len(partners)
            if len(partners):
                med2[0, s, c], med2[1, s, c] = _median_cell(cor, raw, s, partners)
    return med2, n_valid


def _nearest_class(med_raw, n_valid, levels):
    """Per sample the label of the class with the largest med_raw among the cells with a partner; ties go to the class
    that is earlier in `levels`; None when no cell has one."""
    med_raw = np.asarray(med_raw, dtype=np.float64)
    has = np.asarray(n_valid) > 0
    score = np.where(has, med_raw, -np.inf)
    best = np.argmax(score, axis=1) if score.shape[1] else np.zeros(score.shape[0], dtype=np.intp)   # (the first maximum)
    return [levels[int(k)] if row.any() else None for k, row in zip(best, has)]


def ici_kendalltau_class_matrix(data_matrix, sample_classes, global_na=(float("nan"), float("inf"), 0),
                                perspective="global", scale_max=True, alternative="two.sided", continuity=False,
                                colnames=None, engine=None):
    """For every sample (column) of a features x samples matrix the median ICI-Kendall-tau to the members of EVERY
    class: the S x C table in which a mislabelled or swapped sample correlates better with another class than with the
    one it is labelled as, and from which a new sample is assigned to its nearest class -- without the S x S matrices
    ``ici_kendalltau`` returns.

    ``sample_classes`` gives one label per column (required); the other arguments are ``ici_kendalltau``'s (column names
    are required; a sparse matrix, float32 and integer matrices are read where they lie).  On the HIP engine the
    reduction runs on the device (icikt_class_matrix_f64); a matrix has at most 65 535 samples and 65 535 classes.

    The partners of cell (s, c) are the samples of class c other than s whose pair with s has a ``raw`` that is not NA
    (the reference's warning is raised once per pair of reasons 2-4, over all pairs).  ``med_raw`` is R's
    ``median(raw, na.rm = TRUE)`` over them and ``med_cor`` the same over ``cor``; with ``scale_max`` ``cor`` is ``raw``
    over the largest ``taumax`` of ALL S (S - 1) / 2 pairs, as in ``ici_kendalltau``.  A cell without a partner (the own
    cell of a singleton among them) is NA.  The own-class column is ``ici_kendalltau_medians``' ``med_raw``.  Returns a
    dict: ``sample_id`` and ``sample_class`` (names and labels in column order), ``classes`` (the levels, in the column
    order of the tables), ``med_cor``, ``med_raw``, ``n_valid`` (S x C each), ``nearest_class`` (per sample the label
    of the class with the largest ``med_raw`` among the cells with a partner, ties to the earlier class, None without
    one), ``max_taumax`` and ``run_time``.
    """
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    if sample_classes is None:
        raise ValueError("`sample_classes` must give one class per column")
    levels, cls = _class_levels(sample_classes, n_sample, "all")
    _need_pairs(n_sample)
    eng = engine or _default_engine()
    if hasattr(eng, "class_matrix"):
        (med2, n_valid, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.class_matrix(X, cls, len(levels), gna, perspective, alternative, continuity, 0, scale_max))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, scale_max, alternative,
                                               continuity)
        med2, n_valid = _class_matrix_numpy(mats5[0], mats5[1], cls, len(levels))
    labels = [levels[k] for k in cls]
    return {"sample_id": list(names), "sample_class": labels, "classes": list(levels), "med_cor": med2[0],
            "med_raw": med2[1], "n_valid": n_valid, "nearest_class": _nearest_class(med2[1], n_valid, levels),
            "max_taumax": max_taumax, "run_time": t_diff}


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_quantiles: exact quantiles and a histogram of raw over all pairs (the cut-off ici_kendalltau_edges is
# called with, the distribution a quality-control report draws; the reference leaves both to the user)
# --------------------------------------------------------------------------------------------------
def _type7(a, b, index, lo):
    """R's quantile(type = 7) between the order statistics a = x[lo] and b = x[hi]: every product and sum rounded on its
    own, a zero as +0."""
    if index == lo or a == b:
        return a + 0.0
    h = index - lo
    wa = (1.0 - h) * a
    wb = h * b
    return (wa + wb) + 0.0


def _quantiles_numpy(cor, raw, cls, probs, breaks):
    """The reduction of icikt_quantiles_f64 from full S x S cor and raw matrices, for engines without a quantiles
    method (the CPU tests' checker engines).  Groups: every pair i < j; with cls also the pairs with cls[i] == cls[j]
    and those with cls[i] != cls[j].  A pair whose raw is NA is no value (n_na).  With the v valid raw values of a group
    ascending x[1..v] (a zero counts as +0) and index = 1 + (v - 1) p, order2 holds x[floor(index)] and x[ceil(index)],
    quantile_raw is R's type 7 between them and quantile_cor the same rule on the cor cells of those two pairs; NA_real_
    when v = 0.  hist is numpy.histogram(valid raw, bins=breaks), outside the values below the first and above the last
    break.  Returns (q2 [2, G, n_probs]: cor, raw; order2 [G, n_probs, 2]; n_valid, n_na [G]; hist [G, n_bins];
    outside [G, 2])."""
    cor = np.ascontiguousarray(cor, dtype=np.float64)
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64)).ravel()
    S = raw.shape[0]
    iu, ju = np.triu_indices(S, k=1)
    with np.errstate(invalid="ignore"):      # (NA_real_ is a signalling NaN)
        r, c = raw[iu, ju] + 0.0, cor[iu, ju] + 0.0
    if cls is None:
        members = [np.ones(r.shape[0], dtype=bool)]
    else:
        cls = np.asarray(cls)
        same = cls[iu] == cls[ju]
        members = [np.ones(r.shape[0], dtype=bool), same, ~same]
    G, n_probs = len(members), probs.shape[0]
    n_bins = 0 if breaks is None else len(breaks) - 1
    q2, order2 = _na_filled((2, G, n_probs)), _na_filled((G, n_probs, 2))
    n_valid, n_na = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    hist, outside = np.zeros((G, n_bins), dtype=np.int64), np.zeros((G, 2), dtype=np.int64)
    for g, member in enumerate(members):
        ok = member & ~np.isnan(r)
        x, xc = r[ok], c[ok]
        v = x.shape[0]
        n_valid[g], n_na[g] = v, int(member.sum()) - v
        if n_bins:
            hist[g] = np.histogram(x, bins=np.asarray(breaks, dtype=np.float64))[0]
            outside[g] = int(np.sum(x < breaks[0])), int(np.sum(x > breaks[-1]))
        if v == 0:
            continue
        order = np.argsort(x, kind="stable")
        for k, p in enumerate(probs):
            index = 1.0 + float(v - 1) * float(p)
            lo, hi = math.floor(index), math.ceil(index)
            a, b = order[lo - 1], order[hi - 1]
            order2[g, k] = x[a], x[b]
            q2[1, g, k] = _type7(float(x[a]), float(x[b]), index, float(lo))
            q2[0, g, k] = _type7(float(xc[a]), float(xc[b]), index, float(lo))
    return q2, order2, n_valid, n_na, hist, outside


def ici_kendalltau_quantiles(data_matrix, probs=(0, 0.25, 0.5, 0.75, 1), breaks=200, sample_classes=None,
                             global_na=(float("nan"), float("inf"), 0), perspective="global", scale_max=True,
                             alternative="two.sided", continuity=False, colnames=None, engine=None):
    """Exact quantiles and a histogram of the ICI-Kendall-tau of ALL S (S - 1) / 2 pairs of samples (columns) of a
    features x samples matrix, without the S x S matrices ``ici_kendalltau`` returns: the 99th percentile
    ``ici_kendalltau_edges`` is called with, and the distribution a quality-control report draws.

    ``probs``: up to 32 probabilities in [0, 1], any order, repeats allowed.  ``breaks``: an int for that many equal bins
    over [-1, 1] (``np.linspace(-1.0, 1.0, breaks + 1)``), an array of strictly increasing bin edges, used as given,
    or None for no histogram; at most 1 024 bins.  ``sample_classes`` gives one label per column and splits the result
    into the groups ``["all", "within", "between"]`` (pairs of one class, pairs across classes); without it the one
    group is ``["all"]``.  The other arguments are ``ici_kendalltau``'s (column names are required; a sparse matrix,
    float32 and integer matrices are read where they lie).  On the HIP engine the reduction runs on the device
    (icikt_quantiles_f64); a matrix has at most 65 535 samples.

    A pair whose ``raw`` is NA is no value (the reference's warning is raised once per pair of reasons 2-4) and counts
    in ``n_na``.  ``quantile_raw`` is R's ``quantile(raw, probs, type = 7, na.rm = TRUE)`` -- numpy's "linear" method --
    over a group's values, exactly: the two order statistics are selected, not estimated.  ``quantile_cor`` is the same
    over ``cor``; with ``scale_max`` ``cor`` is ``raw`` over the largest ``taumax`` of all pairs.  A group without a
    value gets NA.  ``counts`` is ``numpy.histogram(raw, bins=breaks)`` per group (the last bin is closed on the right),
    ``n_below`` and ``n_above`` count the values outside the breaks.  Returns a dict: ``probs``, ``group``,
    ``quantile_cor``, ``quantile_raw`` (n_group x n_probs), ``n_valid``, ``n_na`` (n_group), ``breaks`` (None without
    a histogram), ``counts`` (n_group x n_bins), ``n_below``, ``n_above``, ``max_taumax`` and ``run_time``.
    """
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    if sample_classes is None:
        levels, cls, groups = ["all"], None, ["all"]
    else:
        levels, cls = _class_levels(sample_classes, n_sample, "all")
        groups = ["all", "within", "between"]
    _need_pairs(n_sample)
    probs_a = np.atleast_1d(np.asarray(probs, dtype=np.float64)).ravel()
    if probs_a.shape[0] > _lib.QUANTILE_MAX_PROBS or not np.all((probs_a >= 0) & (probs_a <= 1)):
        raise ValueError(f"`probs` must be at most {_lib.QUANTILE_MAX_PROBS} values in [0, 1]")
    if breaks is None:
        breaks_a = None
    else:
        if isinstance(breaks, (int, np.integer)) and not isinstance(breaks, (bool, np.bool_)):
            if not 1 <= int(breaks) <= _lib.HIST_MAX_BINS:
                raise ValueError(f"`breaks` as a number of bins must be in 1 .. {_lib.HIST_MAX_BINS}")
            breaks_a = np.linspace(-1.0, 1.0, int(breaks) + 1)
        else:
            breaks_a = np.ascontiguousarray(np.atleast_1d(breaks), dtype=np.float64).ravel()
        if not 2 <= breaks_a.shape[0] <= _lib.HIST_MAX_BINS + 1 or not np.all(np.isfinite(breaks_a)) \
                or not np.all(np.diff(breaks_a) > 0):
            raise ValueError(f"`breaks` must be 2 .. {_lib.HIST_MAX_BINS + 1} finite, strictly increasing bin edges")
    eng = engine or _default_engine()
    if hasattr(eng, "quantiles"):
        (q2, _order2, n_valid, n_na, hist, outside, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.quantiles(X, probs_a, breaks_a, cls, len(levels), gna, perspective, alternative,
                                         continuity, 0, scale_max))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, scale_max, alternative,
                                               continuity)
        q2, _order2, n_valid, n_na, hist, outside = _quantiles_numpy(mats5[0], mats5[1], cls, probs_a, breaks_a)
    return {"probs": probs_a, "group": groups, "quantile_cor": q2[0], "quantile_raw": q2[1], "n_valid": n_valid,
            "n_na": n_na, "breaks": breaks_a, "counts": hist, "n_below": outside[:, 0].copy(),
            "n_above": outside[:, 1].copy(), "max_taumax": max_taumax, "run_time": t_diff}


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_edges: every pair past a threshold, the edge list of a correlation network (the reference's
# return_matrix = FALSE data.frame and cor_matrix_2_long_df are its unfiltered form)
# --------------------------------------------------------------------------------------------------
EDGES_DEFAULT_CAPACITY = 2 ** 20   # max_edges=None: the first call has room for max(this, EDGES_CAPACITY_PER_SAMPLE x S)
EDGES_CAPACITY_PER_SAMPLE = 32     # edges (and never more than the triangle holds)


def _edge_bound(value, name):
    if value is None:
        return None
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"`{name}` must be a number or None")
    if math.isnan(float(value)):
        raise ValueError(f"`{name}` must not be NaN (None means no bound)")
    return float(value)


def _candidate_triangle(mats5, min_raw, absolute=False):
    """The upper triangle of five full S x S matrices (cor, raw, pvalue, taumax, completeness) in combn order -- row-
    major: i ascending, then j ascending -- and its candidate pairs: raw not NA, and raw (abs(raw) with absolute) >=
    min_raw when that is not None, as a plain comparison of doubles.  Returns (iu: the triangle's indices; tri5 [5, P]:
    the planes there; ok [P]: the candidates)."""
    mats5 = [np.ascontiguousarray(m, dtype=np.float64) for m in mats5]
    S = mats5[1].shape[0]
    iu = np.triu_indices(S, k=1)
    tri5 = np.stack([m[iu] for m in mats5]) if S > 1 else np.empty((5, 0))
    raw = tri5[1]
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(raw)
        if min_raw is not None:
            ok &= (np.abs(raw) if absolute else raw) >= min_raw
    return iu, tri5, ok


def _edges_numpy(mats5, min_raw, max_pvalue, min_completeness, absolute):
    """The selection of icikt_edges_f64 from five full S x S matrices (cor, raw, pvalue, taumax, completeness), for
    engines without an edges method (the CPU tests' checker engines): the upper triangle in combn order, raw not NA and
    every bound that is not None, as plain comparisons of doubles.  Returns (ei, ej, vals5 [5, m], degree [S]): all of
    the matching pairs."""
    S = np.shape(mats5[1])[0]
    iu, tri5, ok = _candidate_triangle(mats5, min_raw, absolute)
    with np.errstate(invalid="ignore"):
        if max_pvalue is not None:
            ok &= tri5[2] <= max_pvalue
        if min_completeness is not None:
            ok &= tri5[4] >= min_completeness
    ei, ej = iu[0][ok].astype(np.int32), iu[1][ok].astype(np.int32)
    degree = np.bincount(ei, minlength=S).astype(np.int64) + np.bincount(ej, minlength=S).astype(np.int64)
    return ei, ej, tri5[:, ok], degree


def ici_kendalltau_edges(data_matrix, min_raw=None, max_pvalue=None, min_completeness=None, absolute=False,
                         max_edges=None, global_na=(float("nan"), float("inf"), 0), perspective="global",
                         scale_max=True, alternative="two.sided", continuity=False, colnames=None, engine=None):
    """Every pair of samples (columns) of a features x samples matrix whose ICI-Kendall-tau passes a cut-off: the edge
    list of a correlation network, without the S x S matrices ``ici_kendalltau`` returns.

    A pair i < j is an edge iff its ``raw`` is not NA and every bound that is not None holds: ``raw >= min_raw``
    (``abs(raw) >= min_raw`` with ``absolute``), ``pvalue <= max_pvalue``, ``completeness >= min_completeness`` (a NaN
    p-value fails a p-value bound).  The bounds apply to ``raw``, never to the scaled ``cor``: its denominator, the
    largest ``taumax`` of all pairs, is known only once every pair has been computed.  Edges come in ``combn`` order (i
    ascending, then j ascending).  The other arguments are ``ici_kendalltau``'s (column names are required; a sparse
    matrix, float32 and integer matrices are read where they lie).  On the HIP engine the compaction runs on the device
    (icikt_edges_f64), its cost and its memory follow the number of edges, not S x S; a matrix has at most 65 535 samples.

    ``max_edges=None`` returns every edge: the first call has room for ``max(2**20, 32 S)`` of them, and when there are
    more the call is repeated ONCE with room for all -- the whole computation twice, with the same result (it is a pure
    function of the input); pass a ``max_edges`` that fits to avoid that.  An explicit ``max_edges`` truncates the list
    in ``combn`` order; ``n_edges`` and ``degree`` still count every matching pair.

    Returns a dict: ``s1``, ``s2`` (the samples' names), ``i``, ``j`` (their indices), ``cor, raw, pvalue, taumax,
    completeness`` (one value per edge), ``n_edges``, ``degree`` (S: matching pairs per sample), ``max_taumax`` and
    ``run_time``.  ``formats.edges_to_coo`` turns it into a sparse matrix.  The reference's warning is raised once per
    pair whose ``raw`` is NA for reasons 2-4, as ``ici_kendalltau_topk`` raises it.
    """
    min_raw = _edge_bound(min_raw, "min_raw")
    max_pvalue = _edge_bound(max_pvalue, "max_pvalue")
    min_completeness = _edge_bound(min_completeness, "min_completeness")
    if max_edges is not None:
        max_edges = _int_arg(max_edges, 0, math.inf, "`max_edges` must be a non-negative integer or None")
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    _need_pairs(n_sample)
    total = n_sample * (n_sample - 1) // 2
    eng = engine or _default_engine()
    if hasattr(eng, "edges"):
        room = min(total, max(EDGES_DEFAULT_CAPACITY, EDGES_CAPACITY_PER_SAMPLE * n_sample)) if max_edges is None else max_edges

        def call(X, gna):
            out = eng.edges(X, min_raw, max_pvalue, min_completeness, absolute, room, gna, perspective, alternative,
                            continuity, 0, scale_max)
            if max_edges is None and out[3] > room:   # the second call is exact: the count does not depend on the room
                out = eng.edges(X, min_raw, max_pvalue, min_completeness, absolute, out[3], gna, perspective, alternative,
                                continuity, 0, scale_max)
            return out
        (ei, ej, vals, n_edges, degree, max_taumax), t_diff = _on_device(eng, data_matrix, global_na, call)
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, scale_max, alternative,
                                               continuity)
        ei, ej, vals, degree = _edges_numpy(mats5, min_raw, max_pvalue, min_completeness, absolute)
        n_edges = int(ei.shape[0])
        if max_edges is not None:
            ei, ej, vals = ei[:max_edges], ej[:max_edges], vals[:, :max_edges]
    names_arr = np.asarray(list(names), dtype=object)
    res = {"s1": names_arr[ei], "s2": names_arr[ej], "i": ei, "j": ej}
    _put_values(res, vals)
    res["n_edges"] = int(n_edges)
    res["degree"] = degree
    res["max_taumax"] = max_taumax
    res["run_time"] = t_diff
    return res


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_mst: the maximum spanning forest of the samples under raw -- their single-linkage clustering, and the
# connected components of the thresholded network at every cut-off (the reference's workflow ends in a heatmap ordered
# by a dendrogram; it leaves the clustering to hclust on the full matrix)
# --------------------------------------------------------------------------------------------------
def _mst_components(parent):
    """Component labels from a union-find parent array: 0, 1, ... in order of each component's smallest sample."""
    S = len(parent)
    label = np.full(S, -1, dtype=np.int32)
    component = np.empty(S, dtype=np.int32)
    n = 0
    for s in range(S):
        r = s
        while parent[r] != r:
            r = parent[r]
        if label[r] < 0:
            label[r] = n
            n += 1
        component[s] = label[r]
    return component, n


def _mst_numpy(mats5, min_raw):
    """The forest of icikt_mst_f64 from five full S x S matrices (cor, raw, pvalue, taumax, completeness), for engines
    without an mst method (the CPU tests' checker engines): Kruskal over the candidate edges of the upper triangle --
    raw not NA, and raw >= min_raw when that is not None -- in the strict edge order, np.lexsort by raw descending (-0
    equal to +0) and then by the combn index, merged by union-find.  Returns (ti, tj, vals5 [5, n_tree], component [S],
    n_components)."""
    S = np.shape(mats5[1])[0]
    iu, tri5, ok = _candidate_triangle(mats5, min_raw)
    raw = tri5[1]
    cand = np.flatnonzero(ok)                # combn indices, ascending
    order = cand[np.lexsort((cand, -(raw[cand] + 0.0)))]   # (+ 0.0: -0 sorts as +0)
    parent = list(range(S))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    picked = []
    ii, jj = iu[0], iu[1]
    for e in order.tolist():
        if len(picked) == S - 1:
            break
        a, b = find(int(ii[e])), find(int(jj[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            picked.append(e)
    picked = np.asarray(picked, dtype=np.int64)
    ti, tj = ii[picked].astype(np.int32), jj[picked].astype(np.int32)
    component, n_comp = _mst_components(parent)
    return ti, tj, tri5[:, picked], component, n_comp


def ici_kendalltau_mst(data_matrix, min_raw=None, global_na=(float("nan"), float("inf"), 0), perspective="global",
                       scale_max=True, alternative="two.sided", continuity=False, colnames=None, engine=None):
    """The maximum spanning forest of the samples (columns) of a features x samples matrix under their ICI-Kendall-tau:
    the single-linkage clustering of the samples, and the connected components of the correlation network at every
    cut-off, without the S x S matrices ``ici_kendalltau`` returns.

    A pair i < j is a *candidate edge* iff its ``raw`` is not NA, and ``raw >= min_raw`` when ``min_raw`` is given (a
    plain comparison of doubles, as in ``ici_kendalltau_edges``).  The *strict edge order* is: larger ``raw`` first, -0
    equal to +0; equal ``raw`` by the smaller ``combn`` index (i ascending, then j ascending).  The order is total, so
    the maximum spanning forest under it is unique -- a pure function of the input.  Its edges are returned in that
    order, which is Kruskal's order and the single-linkage merge order.  A sample all of whose pairs are NA or below
    ``min_raw`` (a constant or all-missing column) is a component of its own.  This is single linkage; complete and
    average linkage, which need S - 1 dependent updates of an S x S table, are ``ici_kendalltau_hclust``.

    The other arguments are ``ici_kendalltau``'s (column names are required; a sparse matrix, float32 and integer
    matrices are read where they lie).  On the HIP engine the forest is found on the device (icikt_mst_f64); a matrix
    has at most 65 535 samples.

    Returns a dict: ``s1``, ``s2`` (the samples' names), ``i``, ``j`` (their indices, i < j), ``cor, raw, pvalue,
    taumax, completeness`` (one value per tree edge; ``cor = raw / max_taumax`` over all pairs with ``scale_max``),
    ``n_tree``, ``component`` (S: the components of the candidate graph, numbered 0, 1, ... in order of their smallest
    sample, as ``scipy.sparse.csgraph.connected_components`` numbers them), ``n_components`` (``n_tree + n_components
    == S``), ``sample_id``, ``max_taumax`` and ``run_time``.  ``formats.mst_to_linkage`` turns it into a
    ``scipy.cluster.hierarchy`` linkage matrix, ``formats.mst_cut`` into the components at any cut-off.  The
    reference's warning is raised once per pair whose ``raw`` is NA for reasons 2-4, as ``ici_kendalltau_edges`` raises
    it.
    """
    min_raw = _edge_bound(min_raw, "min_raw")
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    _need_pairs(n_sample)
    eng = engine or _default_engine()
    if hasattr(eng, "mst"):
        (ti, tj, vals, component, n_comp, _n_rounds, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.mst(X, min_raw, gna, perspective, alternative, continuity, 0, scale_max))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, scale_max, alternative,
                                               continuity)
        ti, tj, vals, component, n_comp = _mst_numpy(mats5, min_raw)
    names_arr = np.asarray(list(names), dtype=object)
    res = {"s1": names_arr[ti], "s2": names_arr[tj], "i": ti, "j": tj}
    _put_values(res, vals)
    res["n_tree"] = int(ti.shape[0])
    res["component"] = component
    res["n_components"] = int(n_comp)
    res["sample_id"] = names_arr
    res["max_taumax"] = max_taumax
    res["run_time"] = t_diff
    return res


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_hclust: complete, average and single linkage of the samples under raw -- the dendrogram and heatmap
# ordering by the methods R's hclust and scipy default to (the reference leaves them to hclust on the full matrix)
# --------------------------------------------------------------------------------------------------
HCLUST_METHODS = ("complete", "average", "single")


def _hclust_numpy(mats5, method, min_raw):
    """The merges of icikt_hclust_f64 from five full S x S matrices (only raw is read), for engines without an hclust
    method (the CPU tests' checker engines): S - 1 steps over a copy of raw, each an argmax over the upper triangle of
    the live slots -- row-major, so equal similarities go to the smaller a, then the smaller b -- and an update of row
    and column a.  A NaN anywhere between two clusters makes them unmergeable; -0 counts as +0; average is
    (n_a w_a + n_b w_b) / (n_a + n_b) in plain float64 operations.  Returns (ma, mb, msize, mraw, component [S],
    n_components)."""
    if method not in HCLUST_METHODS:
        raise ValueError("`method` must be complete, average or single")
    with np.errstate(invalid="ignore"):
        W = np.array(mats5[1], dtype=np.float64) + 0.0      # (+ 0.0: -0 becomes +0)
    S = W.shape[0]
    np.fill_diagonal(W, np.nan)
    W[np.tril_indices(S)] = np.nan                           # the upper triangle carries the table: W[a, b], a < b
    W = np.fmax(W, W.T)                                      # ... mirrored, so that a row is a slot's similarities
    alive = np.ones(S, dtype=bool)
    size = np.ones(S, dtype=np.int64)
    parent = np.arange(S)
    ma, mb, msize, mraw = [], [], [], []
    for _step in range(S - 1):
        U = np.where(np.triu(alive[:, None] & alive[None, :], k=1), W, np.nan)
        if np.all(np.isnan(U)):
            break
        flat = int(np.nanargmax(U))                          # the first of equal maxima in row-major order
        a, b = divmod(flat, S)
        best = U[a, b]
        if min_raw is not None and not best >= min_raw:
            break
        wa, wb = W[a].copy(), W[b].copy()
        if method == "complete":
            new = np.minimum(wa, wb)                         # (np.minimum propagates NaN)
        elif method == "single":
            new = np.maximum(wa, wb)
        else:
            na, nb = float(size[a]), float(size[b])
            new = (na * wa + nb * wb) / (na + nb) + 0.0
        new[a] = np.nan
        W[a, :] = new
        W[:, a] = new
        alive[b] = False
        size[a] += size[b]
        parent[b] = a
        ma.append(a)
        mb.append(b)
        msize.append(int(size[a]))
        mraw.append(best)
    component, n_comp = _mst_components(parent)
    return (np.asarray(ma, dtype=np.int32), np.asarray(mb, dtype=np.int32), np.asarray(msize, dtype=np.int32),
            np.asarray(mraw, dtype=np.float64), component, n_comp)


def ici_kendalltau_hclust(data_matrix, method="complete", min_raw=None, global_na=(float("nan"), float("inf"), 0),
                          perspective="global", scale_max=True, alternative="two.sided", continuity=False, colnames=None,
                          engine=None):
    """Agglomerative clustering of the samples (columns) of a features x samples matrix under their ICI-Kendall-tau with
    ``"complete"`` (R's ``hclust`` default), ``"average"`` (scipy's and seaborn's) or ``"single"`` linkage, without the
    S x S matrices ``ici_kendalltau`` returns.

    The rule.  The similarity of two samples is the pair's ``raw`` (-0 equal to +0); a pair whose ``raw`` is NA has
    none.  A cluster lives in the slot of its smallest sample, and slot i starts as sample i.  Each step merges the
    best live pair of clusters a < b into a, in a strict order: the larger similarity first, then the smaller a, then
    the smaller b -- a total order, so the result is a pure function of the input.  The merged cluster's similarity to
    a cluster k is NA if either old similarity is NA (two clusters merge only if every sample pair across them has a
    ``raw``), else the smaller of the two (complete), the larger (single), or ``(n_a w_a + n_b w_b) / (n_a + n_b)`` in
    plain doubles (average).  Merging ends at the first step whose best similarity is NA or below ``min_raw``; what is
    left is a forest, its components numbered by their smallest sample.

    The other arguments are ``ici_kendalltau``'s (column names are required; a sparse matrix, float32 and integer
    matrices are read where they lie).  On the HIP engine the steps run on the device (icikt_hclust_f64), which keeps
    12 bytes per cell of an S x S table; a matrix has at most 65 535 samples.

    Returns a dict: ``merge_a``, ``merge_b`` (the slots a < b of each merge, in merge order), ``size`` (the samples of
    the new cluster), ``raw`` (the similarity of the merge), ``cor`` (``raw / max_taumax`` over all pairs with
    ``scale_max``), ``n_merges``, ``component`` (S), ``n_components`` (``n_merges + n_components == S``), ``method``,
    ``sample_id``, ``max_taumax`` and ``run_time``.  ``formats.hclust_to_linkage`` turns it into a
    ``scipy.cluster.hierarchy`` linkage matrix, ``formats.hclust_cut`` into the clusters at any similarity.  The
    reference's warning is raised once per pair whose ``raw`` is NA for reasons 2-4, as ``ici_kendalltau_edges`` raises
    it.
    """
    if method not in HCLUST_METHODS:
        raise ValueError("`method` must be complete, average or single")
    min_raw = _edge_bound(min_raw, "min_raw")
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    _need_pairs(n_sample)
    eng = engine or _default_engine()
    if hasattr(eng, "hclust"):
        (ma, mb, msize, mraw, mcor, component, n_comp, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.hclust(X, method, min_raw, gna, perspective, alternative, continuity, 0, scale_max))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, scale_max, alternative,
                                               continuity)
        ma, mb, msize, mraw, component, n_comp = _hclust_numpy(mats5, method, min_raw)
        mcor = mraw / max_taumax if scale_max else mraw.copy()
    return {"merge_a": ma, "merge_b": mb, "size": msize, "raw": mraw, "cor": mcor, "n_merges": int(ma.shape[0]),
            "component": component, "n_components": int(n_comp), "method": method,
            "sample_id": np.asarray(list(names), dtype=object), "max_taumax": max_taumax, "run_time": t_diff}


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_padjust / ici_kendalltau_significant: R's p.adjust over the p-values of all pairs, and the edges that
# stay significant after it (the reference leaves both to the user: p.adjust(out$pvalue[upper.tri(..)], "BH"))
# --------------------------------------------------------------------------------------------------
PADJUST_METHODS = ("bonferroni", "holm", "hochberg", "BH")   # p.adjust's spelling; "fdr" is its other name for "BH"
PADJUST_DEFAULT_TABLE = 2 ** 20    # max_table=None: distinct p-values the first call has room for


def _padjust_method(method):
    if method in PADJUST_METHODS:
        return method
    if method == "fdr":
        return "BH"
    if method in ("BY", "hommel"):
        raise ValueError(f"`method` {method!r} is not provided (its constants or recursions are not a scan); "
                         f"use one of {', '.join(PADJUST_METHODS)}")
    raise ValueError(f"`method` must be one of {', '.join(PADJUST_METHODS)} (or 'fdr' for BH), spelled as p.adjust "
                     f"spells them, not {method!r}")


def _padjust_alpha(alpha):
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64)).ravel()
    if not 1 <= a.shape[0] <= _lib.ADJUST_MAX_ALPHA or not np.all((a >= 0) & (a <= 1)):
        raise ValueError(f"`alpha` must be 1 .. {_lib.ADJUST_MAX_ALPHA} values in [0, 1]")
    return a


def _padjust_numpy(pvalue_matrix, method, alpha):
    """The reduction of icikt_padjust_f64 from a full S x S p-value matrix, for engines without a padjust method (the
    CPU tests' checker engines).  The tests are the pairs i < j whose p-value is not NaN; sorted ascending, their
    adjusted values are R's p.adjust, one IEEE operation at a time (bonferroni m p, holm cummax((m + 1 - j) p),
    hochberg and BH cummin from the right of (m + 1 - j) p and (m / j) p, each clamped at 1).  Returns (n_tests [2]:
    tests, other pairs; n_rejected [n_alpha]; p_cutoff [n_alpha], NA_real_ where nothing is rejected; table_p,
    table_adjusted: ALL the distinct p-values among the rejected tests of the largest alpha, and their adjusted
    values)."""
    pv = np.ascontiguousarray(pvalue_matrix, dtype=np.float64)
    alpha = np.atleast_1d(np.asarray(alpha, dtype=np.float64)).ravel()
    S = pv.shape[0]
    tri = pv[np.triu_indices(S, k=1)]
    p = np.sort(tri[~np.isnan(tri)] + 0.0)
    m = p.shape[0]
    j = np.arange(1, m + 1, dtype=np.float64)
    if method == "bonferroni":
        adj = float(m) * p
    elif method == "holm":
        adj = np.maximum.accumulate((float(m + 1) - j) * p)
    elif method == "hochberg":
        adj = np.minimum.accumulate(((float(m + 1) - j) * p)[::-1])[::-1]
    else:
        adj = np.minimum.accumulate(((float(m) / j) * p)[::-1])[::-1]
    adj = np.minimum(1.0, adj)
    n_rejected = np.array([int(np.count_nonzero(adj <= a)) for a in alpha], dtype=np.int64)
    p_cutoff = _na_filled(alpha.shape[0])
    for a, n in enumerate(n_rejected):
        if n > 0:
            p_cutoff[a] = p[n - 1]
    most = int(n_rejected.max()) if n_rejected.size else 0
    head = np.ones(most, dtype=bool)
    if most > 1:
        head[1:] = p[1:most] != p[:most - 1]
    return (np.array([m, tri.shape[0] - m], dtype=np.int64), n_rejected, p_cutoff, p[:most][head].copy(),
            adj[:most][head].copy())


def ici_kendalltau_padjust(data_matrix, method="BH", alpha=0.05, max_table=None,
                           global_na=(float("nan"), float("inf"), 0), perspective="global", alternative="two.sided",
                           continuity=False, colnames=None, engine=None):
    """Multiple-testing adjustment of the p-values of ALL S (S - 1) / 2 pairs of samples (columns) of a features x
    samples matrix, without the S x S matrices ``ici_kendalltau`` returns: how many pairs stay significant at each
    ``alpha`` after R's ``p.adjust(p, method)``, and the raw p-value to cut at.

    ``method``: ``"bonferroni"``, ``"holm"``, ``"hochberg"`` or ``"BH"`` (``"fdr"`` is BH), spelled as ``p.adjust``
    spells them; ``"BY"`` and ``"hommel"`` are not provided.  ``alpha``: one level or up to 16, each in [0, 1].  The
    tests are the pairs whose p-value is not NA (a pair whose ``raw`` is NA is none: the reference's warning is raised
    once per pair of reasons 2-4); ``n_tests`` is their count m, ``n_na`` the count of the others.  The adjusted
    values are ``p.adjust``'s to the bit (for BH also ``scipy.stats.false_discovery_control``'s).  The other arguments
    are ``ici_kendalltau``'s (column names are required; a sparse matrix, float32 and integer matrices are read where
    they lie).  On the HIP engine the p-values are sorted, scanned and cut on the device (icikt_padjust_f64); a matrix
    has at most 65 535 samples.

    ``n_rejected[a]`` is the number of tests whose adjusted p-value is ``<= alpha[a]`` and ``p_cutoff[a]`` the largest
    raw p-value among them (NA when there is none): ``adjusted <= alpha[a]`` exactly when ``pvalue <= p_cutoff[a]``, so
    ``ici_kendalltau_edges(max_pvalue=p_cutoff[a])`` returns exactly the rejected pairs (``ici_kendalltau_significant``
    does that).  ``table_p`` holds the distinct p-values among the rejected tests of the largest alpha, ascending, and
    ``table_adjusted`` their adjusted values.  ``max_table=None`` returns the whole table: the first call has room for
    ``2**20`` entries, and when there are more the call is repeated ONCE with room for all -- the whole computation
    twice, with the same result; pass a ``max_table`` that fits to avoid that.  An explicit ``max_table`` truncates
    the table; ``n_table`` still counts every distinct value.

    Returns a dict: ``method``, ``alpha``, ``n_tests``, ``n_na``, ``n_rejected``, ``p_cutoff`` (one value per alpha),
    ``table_p``, ``table_adjusted``, ``n_table``, ``max_taumax`` and ``run_time``.
    """
    method = _padjust_method(method)
    alpha_a = _padjust_alpha(alpha)
    if max_table is not None:
        max_table = _int_arg(max_table, 0, math.inf, "`max_table` must be a non-negative integer or None")
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    _need_pairs(n_sample)
    total = n_sample * (n_sample - 1) // 2
    eng = engine or _default_engine()
    if hasattr(eng, "padjust"):
        room = min(total, PADJUST_DEFAULT_TABLE) if max_table is None else max_table

        def call(X, gna):
            out = eng.padjust(X, method, alpha_a, room, gna, perspective, alternative, continuity, 0)
            if max_table is None and out[4] > room:   # the second call is exact: the count does not depend on the room
                out = eng.padjust(X, method, alpha_a, out[4], gna, perspective, alternative, continuity, 0)
            return out
        (n_tests, n_rejected, p_cutoff, table, n_table, max_taumax), t_diff = _on_device(eng, data_matrix, global_na, call)
        table_p, table_adj = table[0], table[1]
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, True, alternative,
                                               continuity)
        n_tests, n_rejected, p_cutoff, table_p, table_adj = _padjust_numpy(mats5[2], method, alpha_a)
        n_table = int(table_p.shape[0])
        if max_table is not None:
            table_p, table_adj = table_p[:max_table], table_adj[:max_table]
    return {"method": method, "alpha": alpha_a, "n_tests": int(n_tests[0]), "n_na": int(n_tests[1]),
            "n_rejected": n_rejected, "p_cutoff": p_cutoff, "table_p": table_p, "table_adjusted": table_adj,
            "n_table": int(n_table), "max_taumax": max_taumax, "run_time": t_diff}


def ici_kendalltau_significant(data_matrix, alpha=0.05, method="BH", min_raw=None, min_completeness=None, absolute=False,
                               max_edges=None, global_na=(float("nan"), float("inf"), 0), perspective="global",
                               scale_max=True, alternative="two.sided", continuity=False, colnames=None, engine=None):
    """The pairs of samples whose ICI-Kendall-tau stays significant at ``alpha`` after ``p.adjust(p, method)`` over all
    S (S - 1) / 2 pairs: the edge list of ``ici_kendalltau_edges`` with an ``adjusted`` column.

    It COMPUTES ALL PAIRS TWICE: ``ici_kendalltau_padjust`` finds the raw p-value to cut at (``p_cutoff``), then
    ``ici_kendalltau_edges`` is called with ``max_pvalue = p_cutoff`` and the caller's ``min_raw``, ``min_completeness``,
    ``absolute`` and ``max_edges``; each edge's adjusted p-value is looked up in the first call's table by the bits of
    its p-value (every edge's p-value is in that table by construction; an error is raised if one is not).  When
    nothing is rejected the empty edge list is returned without the second call.  The adjustment is over ALL pairs with
    a p-value, whatever the other bounds keep.

    Returns ``ici_kendalltau_edges``' dict plus ``adjusted`` (one value per edge), ``alpha``, ``method``, ``n_tests``,
    ``n_rejected`` and ``p_cutoff``; ``run_time`` is the sum of the two calls.
    """
    if isinstance(alpha, (bool, np.bool_)) or not isinstance(alpha, (int, float, np.integer, np.floating)) \
            or not 0 <= float(alpha) <= 1:
        raise ValueError("`alpha` must be one number in [0, 1]")
    data_matrix, names = _as_matrix(data_matrix, colnames, "data_matrix", keep_dtype=True, keep_sparse=True)
    adj = ici_kendalltau_padjust(data_matrix, method=method, alpha=float(alpha), max_table=None, global_na=global_na,
                                 perspective=perspective, alternative=alternative, continuity=continuity,
                                 colnames=names, engine=engine)
    n_rejected, p_cutoff = int(adj["n_rejected"][0]), float(adj["p_cutoff"][0])
    if n_rejected == 0:
        none_i = np.empty(0, dtype=np.int32)
        res = {"s1": np.empty(0, dtype=object), "s2": np.empty(0, dtype=object), "i": none_i, "j": none_i.copy()}
        _put_values(res, np.empty((5, 0), dtype=np.float64))
        res.update(n_edges=0, degree=np.zeros(data_matrix.shape[1], dtype=np.int64), max_taumax=adj["max_taumax"],
                   run_time=adj["run_time"], adjusted=np.empty(0, dtype=np.float64))
    else:
        with warnings.catch_warnings():   # (the first call has raised the pairs' warnings)
            warnings.simplefilter("ignore")
            res = ici_kendalltau_edges(data_matrix, min_raw=min_raw, max_pvalue=p_cutoff,
                                       min_completeness=min_completeness, absolute=absolute, max_edges=max_edges,
                                       global_na=global_na, perspective=perspective, scale_max=scale_max,
                                       alternative=alternative, continuity=continuity, colnames=names, engine=engine)
        # p-values are >= 0 and a zero is +0 on both sides: the order of the bits is the order of the values
        table_bits = np.ascontiguousarray(adj["table_p"], dtype=np.float64).view(np.uint64)
        edge_bits = (np.ascontiguousarray(res["pvalue"], dtype=np.float64) + 0.0).view(np.uint64)
        at = np.searchsorted(table_bits, edge_bits)
        if np.any(at >= table_bits.shape[0]) or np.any(table_bits[np.minimum(at, table_bits.shape[0] - 1)] != edge_bits):
            raise RuntimeError("ici_kendalltau_significant: an edge's p-value is not among the adjusted p-values")
        res["adjusted"] = np.asarray(adj["table_adjusted"], dtype=np.float64)[at]
        res["run_time"] = res["run_time"] + adj["run_time"]
    res.update(alpha=float(alpha), method=adj["method"], n_tests=adj["n_tests"], n_rejected=n_rejected,
               p_cutoff=p_cutoff)
    return res


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_anosim: do the classes separate under ICI-Kt?  Analysis of similarities (Clarke 1993; vegan::anosim)
# on the dissimilarity 1 - raw with its permutation test (the reference leaves it to vegan on the S x S matrix)
# --------------------------------------------------------------------------------------------------
def _na_real():
    return float(np.array([_NA_REAL_BITS], dtype=np.uint64).view(np.float64)[0])


def anosim_statistic(M, w2, nw):
    """ANOSIM's R of one labelling as an exact ``Fraction``, from the integers of icikt_anosim_f64: M values, w2 the
    doubled rank sum and nw the count of the within-class values.  R = (T2 nw - w2 M) / (nw nB M) with T2 = M (M + 1)
    and nB = M - nw, which is ((M + 1) nw - w2) / (nw nB).  None when nw = 0 or nB = 0: R is undefined."""
    M, w2, nw = int(M), int(w2), int(nw)
    if nw <= 0 or nw >= M:
        return None
    return Fraction((M + 1) * nw - w2, nw * (M - nw))


def anosim_permutations(codes, permutations=999, seed=None, strata=None):
    """The labellings ``ici_kendalltau_anosim`` compares with, [n_perm, S] int32, from the class codes of the columns.
    THE CONTRACT: ``rng = numpy.random.default_rng(seed)`` is made once; permutation t = 0, 1, .. is
    ``rng.permutation(codes)``, drawn in this sequence.  With ``strata`` (a label per column) permutation t starts as
    a copy of ``codes``, and for every stratum, the strata in order of first appearance, the codes at the stratum's
    columns (ascending) are replaced by ``rng.permutation`` of them, on the same stream.  An integer array
    ``permutations`` of shape [n_perm, S] is returned as given (as int32); ``seed`` and ``strata`` are then unused."""
    codes = np.ascontiguousarray(codes, dtype=np.int32).ravel()
    S = codes.shape[0]
    if not isinstance(permutations, (int, np.integer)) or isinstance(permutations, (bool, np.bool_)):
        perms = np.asarray(permutations)
        if perms.ndim != 2 or perms.shape[1] != S or not np.issubdtype(perms.dtype, np.integer):
            raise ValueError("`permutations` must be a count or an integer array [n_perm, S] of class codes")
        return np.ascontiguousarray(perms, dtype=np.int32)
    n_perm = int(permutations)
    if n_perm < 0 or n_perm > _lib.ANOSIM_MAX_PERM:
        raise ValueError(f"`permutations` must be in 0 .. {_lib.ANOSIM_MAX_PERM}")
    groups = None
    if strata is not None:
        labels = list(np.asarray(strata, dtype=object).ravel())
        if len(labels) != S:
            raise ValueError("`strata` must give one stratum per column")
        where = {}
        for s, v in enumerate(labels):   # (a dict keeps the order of first appearance)
            where.setdefault(v, []).append(s)
        groups = [np.asarray(ix, dtype=np.intp) for ix in where.values()]
    rng = np.random.default_rng(seed)
    out = np.empty((n_perm, S), dtype=np.int32)
    for t in range(n_perm):
        if groups is None:
            out[t] = rng.permutation(codes)
        else:
            out[t] = codes
            for ix in groups:
                out[t, ix] = rng.permutation(codes[ix])
    return out


def _labellings_input(data_matrix, colnames, sample_classes, permutations, seed, strata):
    """The start of the two permutation tests: the matrix and its names, the required classes as levels and codes, at
    least two samples, the labellings to compare with.  Returns (data_matrix, names, n_sample, levels, cls, perms)."""
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    if sample_classes is None:
        raise ValueError("`sample_classes` must give one class per column")
    levels, cls = _class_levels(sample_classes, n_sample, "all")
    _need_pairs(n_sample)
    return data_matrix, names, n_sample, levels, cls, anosim_permutations(cls, permutations, seed, strata)


def _as_float(f):
    """A Fraction or an int as a double, None as NA (Fraction -> float rounds correctly, once)."""
    return _na_real() if f is None else float(f)


def _labellings_result(head, counts, before_perms, perm_stats, after_perms, levels, own, names, max_taumax, t_diff):
    """The result dict of the two permutation tests, in its order; counts: (n_perm, n_ge, n_undefined); perm_stats: the
    permutations' statistics as fractions (None: not asked for), between what the test puts before and after them."""
    n_perm, n_ge, n_undef = counts
    res = dict(head, n_permutations=n_perm, n_ge=int(n_ge), n_undefined=int(n_undef), **before_perms)
    if perm_stats is not None:
        res["perm_statistic"] = np.array([_as_float(f) for f in perm_stats], dtype=np.float64)
    res.update(after_perms, class_levels=list(levels), **own, sample_id=list(names), max_taumax=max_taumax, run_time=t_diff)
    return res


def _anosim_numpy(raw, cls, n_class, perms):
    """The sums of icikt_anosim_f64 from a full S x S raw matrix, for engines without an anosim method (the CPU tests'
    checker engines): (n_pairs [2], w2, nw [1 + n_perm], n_ge, n_undefined, class_w2, class_nw [n_class])."""
    raw = np.asarray(raw, dtype=np.float64)
    S = raw.shape[0]
    iu, ju = np.triu_indices(S, k=1)
    v = raw[iu, ju]
    ok = ~np.isnan(v)
    iu, ju, v = iu[ok], ju[ok], v[ok] + 0.0
    M = int(v.shape[0])
    asc = np.sort(v)
    r2 = (2 * M - np.searchsorted(asc, v, "left") - np.searchsorted(asc, v, "right") + 1).astype(np.int64)
    labs = np.vstack([np.asarray(cls, dtype=np.int64)[None, :], np.asarray(perms, dtype=np.int64).reshape(-1, S)])
    w2 = np.zeros(labs.shape[0], dtype=np.int64)
    nw = np.zeros(labs.shape[0], dtype=np.int64)
    for q, lab in enumerate(labs):
        same = lab[iu] == lab[ju]
        w2[q], nw[q] = r2[same].sum(), same.sum()
    obs = anosim_statistic(M, w2[0], nw[0])
    stats = [anosim_statistic(M, a, b) for a, b in zip(w2[1:], nw[1:])]
    n_ge = sum(1 for f in stats if f is not None and obs is not None and f >= obs)
    n_undef = sum(1 for f in stats if f is None)
    same = labs[0][iu] == labs[0][ju]
    class_w2 = np.zeros(n_class, dtype=np.int64)
    np.add.at(class_w2, labs[0][iu][same], r2[same])
    class_nw = np.bincount(labs[0][iu][same], minlength=n_class).astype(np.int64)
    return np.array([M, S * (S - 1) // 2 - M], dtype=np.int64), w2, nw, n_ge, n_undef, class_w2, class_nw


def ici_kendalltau_anosim(data_matrix, sample_classes, permutations=999, seed=None, strata=None, return_perms=True,
                          global_na=(float("nan"), float("inf"), 0), perspective="global", alternative="two.sided",
                          continuity=False, colnames=None, engine=None):
    """Do the classes of the samples (columns) of a features x samples matrix separate under ICI-Kendall-tau, and how
    sure is that: analysis of similarities (Clarke 1993; ``vegan::anosim``) on the dissimilarity ``1 - raw`` with its
    permutation test -- without the S x S matrices ``ici_kendalltau`` returns.

    ``sample_classes`` gives one label per column (required; the levels are ``ici_kendalltau_class_matrix``'s, in the
    same order).  A pair is a value when its ``raw`` is not NA (the reference's warning is raised once per pair of
    reasons 2-4); the M values are ranked by ascending ``1 - raw``, that is descending ``raw``, ties by their average
    (-0 equals +0).  The statistic is R = (mean rank between classes - mean rank within classes) / (M / 2); it is 1 when
    every within-class pair correlates better than every between-class pair, about 0 when the labels say nothing.  R is
    undefined (NA) without a within-class or without a between-class value.

    THE PERMUTATIONS are fixed by (input, ``seed``): ``rng = numpy.random.default_rng(seed)`` is made once and
    permutation t is ``rng.permutation(codes)`` of the columns' class codes, drawn in sequence; with ``strata`` (a label
    per column) the codes are permuted within each stratum, the strata in order of first appearance, on the same stream
    (``anosim_permutations`` is that rule).  ``permutations`` is their number (999, at most 1 000 000) or an integer
    array [n_perm, S] of class codes used as given.  ``pvalue`` is ``(1 + n_ge) / (1 + n_perm)`` with ``n_ge`` the
    permutations whose R is defined and ``>=`` the observed R -- compared exactly, as fractions of integers, so no
    margin like vegan's ``sqrt(.Machine$double.eps)`` is subtracted; ``n_undefined`` permutations have no R and do not
    count.  ``statistic``, ``pvalue`` and every other double come from the integers by one correctly rounded
    conversion.  On the HIP engine ranks and sums are computed on the device (icikt_anosim_f64); a matrix has at most
    65 535 samples.  The other arguments are ``ici_kendalltau``'s (column names are required; a sparse matrix, float32
    and integer matrices are read where they lie).

    Returns a dict: ``statistic``, ``pvalue`` (NA when the observed R is undefined), ``n_permutations``, ``n_ge``,
    ``n_undefined``, ``n_valid`` (M), ``n_na``, ``perm_statistic`` ([n_perm], NA where undefined; only with
    ``return_perms``), ``class_levels``, ``class_mean_rank`` (per class the mean rank of its within-class values, NA
    without one), ``within_mean_rank``, ``between_mean_rank``, ``sums`` (the integers: ``w2``, ``nw`` [1 + n_perm],
    index 0 the observed labelling, ``class_w2``, ``class_nw``), ``sample_id``, ``max_taumax`` and ``run_time``.
    """
    data_matrix, names, n_sample, levels, cls, perms = _labellings_input(data_matrix, colnames, sample_classes,
                                                                         permutations, seed, strata)
    eng = engine or _default_engine()
    if hasattr(eng, "anosim"):
        (n_pairs, w2, nw, n_ge, n_undef, class_w2, class_nw, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.anosim(X, cls, len(levels), perms, gna, perspective, alternative, continuity, 0))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, True, alternative,
                                               continuity)
        n_pairs, w2, nw, n_ge, n_undef, class_w2, class_nw = _anosim_numpy(mats5[1], cls, len(levels), perms)
    M, n_perm = int(n_pairs[0]), int(perms.shape[0])
    obs = anosim_statistic(M, w2[0], nw[0])
    W2, nW = int(w2[0]), int(nw[0])
    return _labellings_result(
        {"statistic": _as_float(obs), "pvalue": _na_real() if obs is None else float(Fraction(1 + int(n_ge), 1 + n_perm))},
        (n_perm, n_ge, n_undef), {"n_valid": M, "n_na": int(n_pairs[1])},
        [anosim_statistic(M, a, b) for a, b in zip(w2[1:], nw[1:])] if return_perms else None, {}, levels,
        {"class_mean_rank": np.array([_as_float(Fraction(int(a), 2 * int(b)) if b else None)
                                      for a, b in zip(class_w2, class_nw)], dtype=np.float64),
         "within_mean_rank": _as_float(Fraction(W2, 2 * nW) if nW else None),
         "between_mean_rank": _as_float(Fraction(M * (M + 1) - W2, 2 * (M - nW)) if M > nW else None),
         "sums": {"w2": w2, "nw": nw, "class_w2": class_w2, "class_nw": class_nw}},
        names, max_taumax, t_diff)


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_permanova: PERMANOVA (Anderson 2001; vegan::adonis2, skbio's permanova) of the classes on the squared
# dissimilarities (1 - raw)^2, summed as fixed-point integers (csrc/icikt_fixed.h)
# --------------------------------------------------------------------------------------------------
PERMANOVA_FRAC_BITS = 50   # fixed::FRAC_BITS: q = (1 - raw)^2 2^50, rounded half to even


def _permanova_quantise(raw):
    """fixed::quantise (csrc/icikt_fixed.h) on an array of raw values without NaN, as int64: -0 is +0, d = 1.0 - raw and
    e = d * d in double, one rounding each, q = rint(ldexp(e, 50))."""
    d = 1.0 - (np.asarray(raw, dtype=np.float64) + 0.0)
    return np.rint(np.ldexp(d * d, PERMANOVA_FRAC_BITS)).astype(np.int64)


class PermanovaStatistic(tuple):
    """(F, r2, ss_total, ss_within, ss_among, df_among, df_within) of one labelling: exact ``Fraction``s and ints.  F is
    None where it is undefined and ``math.inf`` when SS_W = 0 < SS_A; r2 is None when SS_T = 0."""
    __slots__ = ()
    F = property(lambda self: self[0])
    r2 = property(lambda self: self[1])
    ss_total = property(lambda self: self[2])
    ss_within = property(lambda self: self[3])
    ss_among = property(lambda self: self[4])
    df_among = property(lambda self: self[5])
    df_within = property(lambda self: self[6])


def _permanova_ss_within(A, sizes):
    """SS_W = sum_c A_c / (n_c 2^50) over the classes with a sample, as one Fraction over the sizes' common multiple."""
    used = [(int(a), int(n)) for a, n in zip(A, sizes) if int(n) > 0]
    L = math.lcm(*(n for _, n in used)) if used else 1
    return Fraction(sum(a * (L // n) for a, n in used), L << PERMANOVA_FRAC_BITS)


def permanova_statistic(S, Q, A, sizes):
    """PERMANOVA's pseudo-F of one labelling, exactly, from the integers of icikt_permanova_f64: S samples, Q the sum of
    q over all pairs, A [n_class] the sums within each class and sizes [n_class] the labelling's class sizes.  With C'
    the classes that have a sample: SS_T = Q / (S 2^50), SS_W = sum_c A_c / (n_c 2^50), SS_A = SS_T - SS_W,
    F = (SS_A / (C' - 1)) / (SS_W / (S - C')) and R2 = SS_A / SS_T.  F is None (undefined) when C' < 2, S <= C' or
    SS_T = 0, and ``math.inf`` when SS_W = 0 < SS_A.  Returns a ``PermanovaStatistic``."""
    S, Q = int(S), int(Q)
    n_used = sum(1 for n in sizes if int(n) > 0)
    ss_t = Fraction(Q, S << PERMANOVA_FRAC_BITS) if S > 0 else Fraction(0)
    ss_w = _permanova_ss_within(A, sizes)
    ss_a = ss_t - ss_w
    df_a, df_w = n_used - 1, S - n_used
    if n_used < 2 or df_w <= 0 or ss_t == 0:
        F = None
    elif ss_w == 0:
        F = math.inf          # (SS_A = SS_T > 0 here)
    else:
        F = (ss_a / df_a) / (ss_w / df_w)
    return PermanovaStatistic((F, ss_a / ss_t if ss_t != 0 else None, ss_t, ss_w, ss_a, df_a, df_w))


def _permanova_compare(S, Q, class_q, labellings, n_class):
    """(the observed labelling's PermanovaStatistic, the permutations' F [n_perm] -- Fraction, None or inf --, n_ge,
    n_undefined) from the integers of every labelling; labellings [1 + n_perm, S], row 0 the observed one.  A
    permutation with the observed class sizes is compared by SS_W alone (S, C' and SS_T are shared: F falls as SS_W
    grows), any other through its F; both exactly."""
    sizes = [np.bincount(lab, minlength=n_class) for lab in labellings]
    obs = permanova_statistic(S, Q, class_q[0], sizes[0])
    Fs, n_ge, n_undef = [], 0, 0
    for a, sz in zip(class_q[1:], sizes[1:]):
        if np.array_equal(sz, sizes[0]):
            if obs.F is None:
                f, ge = None, False
            else:
                ss_w = _permanova_ss_within(a, sz)
                ge = ss_w <= obs.ss_within
                f = math.inf if ss_w == 0 else ((obs.ss_total - ss_w) / obs.df_among) / (ss_w / obs.df_within)
        else:
            f = permanova_statistic(S, Q, a, sz).F
            ge = f is not None and obs.F is not None and f >= obs.F
        Fs.append(f)
        n_undef += f is None
        n_ge += bool(ge)
    return obs, Fs, n_ge, n_undef


def _permanova_numpy(raw, cls, n_class, perms):
    """The integers of icikt_permanova_f64 from a full S x S raw matrix, for engines without a permanova method (the CPU
    tests' checker engines): (n_pairs [2], Q, class_q [1 + n_perm, n_class] of Python ints).  The sums are taken limb by
    limb in int64, as the device takes them."""
    raw = np.asarray(raw, dtype=np.float64)
    S = raw.shape[0]
    iu, ju = np.triu_indices(S, k=1)
    v = raw[iu, ju]
    ok = ~np.isnan(v)
    n_na = int((~ok).sum())
    q = _permanova_quantise(v[ok])
    lo, hi = q & 0xFFFFFFFF, q >> 32
    labs = np.vstack([np.asarray(cls, dtype=np.int64)[None, :], np.asarray(perms, dtype=np.int64).reshape(-1, S)])
    class_q = np.zeros((labs.shape[0], n_class), dtype=object)
    if n_na == 0:
        for l, lab in enumerate(labs):
            same = lab[iu] == lab[ju]
            a_lo, a_hi = np.zeros(n_class, dtype=np.int64), np.zeros(n_class, dtype=np.int64)
            np.add.at(a_lo, lab[iu][same], lo[same])
            np.add.at(a_hi, lab[iu][same], hi[same])
            class_q[l] = a_hi.astype(object) * (1 << 32) + a_lo.astype(object)
    return (np.array([int(ok.sum()), n_na], dtype=np.int64), (int(hi.sum()) << 32) + int(lo.sum()), class_q)


def ici_kendalltau_permanova(data_matrix, sample_classes, permutations=999, seed=None, strata=None, return_perms=True,
                             global_na=(float("nan"), float("inf"), 0), perspective="global",
                             alternative="two.sided", continuity=False, colnames=None, engine=None):
    """Do the class labels of the samples (columns) explain the structure of their ICI-Kendall-tau correlations:
    PERMANOVA (Anderson 2001; ``vegan::adonis2``, ``skbio.stats.distance.permanova``) on the dissimilarity ``1 - raw``,
    with its permutation test -- without the S x S matrices ``ici_kendalltau`` returns.  It is the test to report beside
    ``ici_kendalltau_anosim``, which is the more sensitive of the two to unequal dispersion (Anderson & Walsh 2013).

    ``sample_classes`` gives one label per column (required; the levels are ``ici_kendalltau_class_matrix``'s).  The sums
    of squares partition the squared dissimilarities: ``ss_total`` is their sum over all pairs divided by S,
    ``ss_within`` the sum over the classes of the within-class pairs' sum divided by the class size, ``ss_among`` the
    difference; ``statistic`` is the pseudo-F ``(ss_among / df_among) / (ss_within / df_within)`` and ``r2`` is
    ``ss_among / ss_total``, the share of the structure the labels explain.  F is NA with fewer than two classes, with
    only singleton classes or when every dissimilarity is 0, and Inf when the classes have no spread at all.

    EXACTNESS.  Every ``(1 - raw)^2`` is turned into an integer multiple of 2^-50 by one fixed rule (two double
    operations and a rounding to even), and everything after that is integer and rational arithmetic: the result is a
    pure function of the input and the labellings, and every double below comes from a fraction by one correctly
    rounded conversion.  F values are compared exactly, so no margin like vegan's ``sqrt(.Machine$double.eps)`` is
    subtracted.

    EVERY PAIR IS NEEDED.  With a pair whose ``raw`` is NA (``n_na > 0``) the class weights have no meaning: nothing is
    imputed and no pair is dropped; every statistic is NA, and one warning says so.  ``ici_kendalltau_medians`` gives
    ``n_valid`` per column, which finds the columns to leave out.

    THE PERMUTATIONS are ``ici_kendalltau_anosim``'s (``anosim_permutations``): the same ``seed`` and ``strata`` give both
    tests the same labellings; an integer array [n_perm, S] of class codes is used as given (its class sizes may differ
    from the observed ones).  ``pvalue`` is ``(1 + n_ge) / (1 + n_perm)`` with ``n_ge`` the labellings whose F is defined
    and ``>=`` the observed F; ``n_undefined`` labellings have no F and do not count.  ``(1 + n_perm)`` times the number of
    classes is at most 2^26.  The other arguments are ``ici_kendalltau``'s (column names are required).

    Returns a dict: ``statistic``, ``r2``, ``pvalue``; ``ss_total``, ``ss_within``, ``ss_among``; ``df_among``,
    ``df_within``; ``n_permutations``, ``n_ge``, ``n_undefined``, ``perm_statistic`` ([n_perm], NA where undefined; only
    with ``return_perms``); ``n_valid``, ``n_na``; ``class_levels``, ``class_size``, ``class_ss`` (per class the
    within-class sum divided by the class size, NA for a class without a sample); ``sums`` (the integers: ``q_total`` and
    ``class_q`` [1 + n_perm, n_class], row 0 the observed labelling); ``sample_id``, ``max_taumax`` and ``run_time``.
    """
    data_matrix, names, n_sample, levels, cls, perms = _labellings_input(data_matrix, colnames, sample_classes,
                                                                         permutations, seed, strata)
    n_class, n_perm = len(levels), int(perms.shape[0])
    if (1 + n_perm) * n_class > _lib.PERMANOVA_MAX_CELLS:
        raise ValueError(f"(1 + permutations) x classes must be at most {_lib.PERMANOVA_MAX_CELLS}")
    if perms.size and (perms.min() < 0 or perms.max() >= n_class):
        raise ValueError("`permutations` holds a class code outside 0 .. n_class - 1")
    eng = engine or _default_engine()
    if hasattr(eng, "permanova"):
        (n_pairs, Q, class_q, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.permanova(X, cls, n_class, perms, gna, perspective, alternative, continuity, 0))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, True, alternative,
                                               continuity)
        n_pairs, Q, class_q = _permanova_numpy(mats5[1], cls, n_class, perms)
    S, n_na = n_sample, int(n_pairs[1])
    sizes = np.bincount(cls, minlength=n_class).astype(np.int64)
    if n_na > 0:
        warnings.warn(f"PERMANOVA needs every pair and {n_na} of them have no raw value: every statistic is NA.  "
                      "`ici_kendalltau_medians` returns `n_valid` per column, which finds the columns to leave out.",
                      RuntimeWarning, stacklevel=2)
        n_used = int((sizes > 0).sum())
        obs = PermanovaStatistic((None, None, None, None, None, n_used - 1, S - n_used))
        Fs, n_ge, n_undef = [None] * n_perm, 0, n_perm
        class_ss = _na_filled(n_class)
    else:
        obs, Fs, n_ge, n_undef = _permanova_compare(S, Q, class_q, np.vstack([cls[None, :], perms]), n_class)
        class_ss = np.array([_as_float(Fraction(int(a), int(n) << PERMANOVA_FRAC_BITS) if n else None)
                             for a, n in zip(class_q[0], sizes)], dtype=np.float64)
    return _labellings_result(
        {"statistic": _as_float(obs.F), "r2": _as_float(obs.r2),
         "pvalue": _na_real() if obs.F is None else float(Fraction(1 + n_ge, 1 + n_perm)),
         "ss_total": _as_float(obs.ss_total), "ss_within": _as_float(obs.ss_within), "ss_among": _as_float(obs.ss_among),
         "df_among": int(obs.df_among), "df_within": int(obs.df_within)},
        (n_perm, n_ge, n_undef), {}, Fs if return_perms else None, {"n_valid": int(n_pairs[0]), "n_na": n_na}, levels,
        {"class_size": sizes, "class_ss": class_ss, "sums": {"q_total": int(Q), "class_q": class_q}},
        names, max_taumax, t_diff)


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_permdisp: PERMDISP (Anderson 2006; vegan::betadisper + permutest) of the classes: every sample's
# distance to the class centroids from the integer table of icikt_permdisp_f64
# --------------------------------------------------------------------------------------------------
_PERMDISP_LIMB = 24   # bits of a limb of the permutation stage: 65 535 of them in a bin stay exact in a double


def permdisp_distance(X, n):
    """The distance of a sample to the centroid of a class of n samples from the integer X = n T - A of the table
    (D^2 = X / (n^2 2^50)): the correctly rounded double of sqrt(|X|) / (n 2^25).  With R = |X| / (n^2 2^50), e chosen
    so that floor(R 4^e) has 127 or 128 bits and m its integer square root (64 bits), m' = 2 m when R 4^e is the
    integer m^2 and 2 m + 1 otherwise: the sticky bit makes the one conversion of m' / 2^(e + 1) round correctly."""
    X, n = abs(int(X)), int(n)
    if n < 1:
        raise ValueError("a centroid needs a class with a sample")
    if X == 0:
        return 0.0
    den = (n * n) << PERMANOVA_FRAC_BITS
    e = (127 - (X.bit_length() - den.bit_length())) // 2
    while True:
        num, d = (X << (2 * e), den) if e >= 0 else (X, den << (-2 * e))
        N, rest = divmod(num, d)
        bits_n = N.bit_length()
        if bits_n < 127:
            e += 1
        elif bits_n > 128:
            e -= 1
        else:
            break
    m = math.isqrt(N)
    m2 = 2 * m if (rest == 0 and m * m == N) else 2 * m + 1
    return float(Fraction(m2, 1 << (e + 1)) if e + 1 >= 0 else Fraction(m2 << -(e + 1)))


class PermdispStatistic(tuple):
    """(F, ss_among, ss_within, df_among, df_within) of one labelling: exact ``Fraction``s and ints.  F is None where
    it is undefined and ``math.inf`` when SS_W = 0 < SS_A."""
    __slots__ = ()
    F = property(lambda self: self[0])
    ss_among = property(lambda self: self[1])
    ss_within = property(lambda self: self[2])
    df_among = property(lambda self: self[3])
    df_within = property(lambda self: self[4])


def _permdisp_ints(values):
    """values (doubles, ints or Fractions) as integers over one denominator: (ints, D) with values[i] = ints[i] / D."""
    fr = [Fraction(v) if not isinstance(v, (float, np.floating)) else Fraction(*float(v).as_integer_ratio()) for v in values]
    D = math.lcm(*(f.denominator for f in fr)) if fr else 1
    return [f.numerator * (D // f.denominator) for f in fr], D


def _permdisp_anova(S, tot, sq, G, sizes):
    """The one-way ANOVA of S integers with sum tot and sum of squares sq whose class sums are G and class sizes
    `sizes`, exactly: (F, SS_A, SS_W, df_among, df_within) in the integers' own unit.  F is None with fewer than two
    classes that have a sample, with S <= C' or when all values are equal, and inf when SS_W = 0 < SS_A."""
    used = [(int(g), int(n)) for g, n in zip(G, sizes) if int(n) > 0]
    L = math.lcm(*(n for _, n in used)) if used else 1
    val = Fraction(sum(g * g * (L // n) for g, n in used), L)      # sum_c G_c^2 / n_c
    ss_a = val - Fraction(tot * tot, S)
    ss_w = sq - val
    df_a, df_w = len(used) - 1, S - len(used)
    if df_a < 1 or df_w <= 0 or S * sq == tot * tot:
        F = None
    elif ss_w == 0:
        F = math.inf
    else:
        F = (ss_a * df_w) / (ss_w * df_a)
    return F, ss_a, ss_w, df_a, df_w


def permdisp_statistic(values, labels, n_class):
    """The one-way ANOVA F of `values` (one per sample: doubles are taken as the rationals they are) over the classes
    `labels` (codes in 0 .. n_class - 1), exactly: with C' the classes that have a sample, F = (SS_A / (C' - 1)) /
    (SS_W / (S - C')).  F is None (undefined) when C' < 2, when S <= C' or when all values are equal, and ``math.inf``
    when SS_W = 0 < SS_A.  Returns a ``PermdispStatistic``."""
    V, D = _permdisp_ints(values)
    lab = [int(c) for c in labels]
    if len(lab) != len(V):
        raise ValueError("`labels` must give one class per value")
    G, sizes = [0] * int(n_class), [0] * int(n_class)
    for v, c in zip(V, lab):
        G[c] += v
        sizes[c] += 1
    F, ss_a, ss_w, df_a, df_w = _permdisp_anova(len(V), sum(V), sum(v * v for v in V), G, sizes)
    return PermdispStatistic((F, ss_a / (D * D), ss_w / (D * D), df_a, df_w))


def _permdisp_permute(residuals, labellings, n_class, F_obs):
    """permutest's stage on the host: the exact ANOVA F of the residuals under every labelling [n_perm, S] (permuting
    residuals over fixed labels is permuting labels over fixed residuals).  The class sums are taken limb by limb
    through ``np.bincount`` -- limbs of 24 bits, at most 65 535 of them in a bin, are exact in a double -- and combined
    as Python ints.  Returns (the F of every labelling -- Fraction, None or inf --, n_ge: those that are defined and
    >= F_obs, compared exactly; n_undefined)."""
    R, _D = _permdisp_ints(residuals)
    S = len(R)
    labellings = np.asarray(labellings, dtype=np.int64).reshape(-1, S)
    tot, sq = sum(R), sum(v * v for v in R)
    off = 1 << max((abs(v).bit_length() for v in R), default=0)          # R + off >= 0
    n_limb = max(1, -(-(off.bit_length() + 1) // _PERMDISP_LIMB))
    mask = (1 << _PERMDISP_LIMB) - 1
    limbs = [np.array([((v + off) >> (_PERMDISP_LIMB * k)) & mask for v in R], dtype=np.float64) for k in range(n_limb)]
    Fs, n_ge, n_undef = [], 0, 0
    step = max(1, (1 << 22) // max(n_class, S))
    for a in range(0, labellings.shape[0], step):
        labs = labellings[a:a + step]
        m = labs.shape[0]
        at = (labs + (np.arange(m, dtype=np.int64) * n_class)[:, None]).ravel()
        sizes = np.bincount(at, minlength=m * n_class).reshape(m, n_class)
        G = -(sizes.astype(object) * off)
        for k, limb in enumerate(limbs):
            part = np.bincount(at, weights=np.tile(limb, m), minlength=m * n_class).astype(np.int64).reshape(m, n_class)
            G = G + part.astype(object) * (1 << (_PERMDISP_LIMB * k))
        for g, sz in zip(G, sizes):
            f = _permdisp_anova(S, tot, sq, g, sz)[0]
            Fs.append(f)
            n_undef += f is None
            n_ge += f is not None and F_obs is not None and f >= F_obs
    return Fs, int(n_ge), int(n_undef)


def _permdisp_numpy(raw, cls, n_class):
    """The integers of icikt_permdisp_f64 from a full S x S raw matrix, for engines without a permdisp method (the CPU
    tests' checker engines): (n_pairs [2], Q, T [S, n_class] of Python ints).  A pair without a value adds 0; the sums
    are taken limb by limb in int64, as the device takes them."""
    raw = np.asarray(raw, dtype=np.float64)
    S = raw.shape[0]
    iu, ju = np.triu_indices(S, k=1)
    v = raw[iu, ju]
    ok = ~np.isnan(v)
    q = np.zeros((S, S), dtype=np.int64)
    q[iu[ok], ju[ok]] = _permanova_quantise(v[ok])
    q = q + q.T
    onehot = (np.asarray(cls, dtype=np.int64)[:, None] == np.arange(n_class, dtype=np.int64)[None, :]).astype(np.int64)
    t_lo, t_hi = (q & 0xFFFFFFFF) @ onehot, (q >> 32) @ onehot
    up = q[iu, ju]
    return (np.array([int(ok.sum()), int((~ok).sum())], dtype=np.int64),
            (int((up >> 32).sum()) << 32) + int((up & 0xFFFFFFFF).sum()),
            t_hi.astype(object) * (1 << 32) + t_lo.astype(object))


def _permdisp_centroids(T, cls, n_class):
    """From the table: (sizes [C], A [C] Python ints, X [S, C] object array of n_c T[i][c] - A_c, 0 in the columns of
    empty classes)."""
    S = T.shape[0]
    sizes = np.bincount(cls, minlength=n_class).astype(np.int64)
    A = []
    for c in range(n_class):
        twice = sum(int(T[i, c]) for i in np.flatnonzero(cls == c))
        if twice % 2:
            raise RuntimeError("ici_kendalltau_permdisp: a class's within-class sum is odd: the table is not symmetric")
        A.append(twice // 2)
    n_obj = np.array([int(n) for n in sizes], dtype=object)
    X = T * n_obj[None, :] - np.array(A, dtype=object)[None, :] if S else np.zeros((0, n_class), dtype=object)
    X[:, sizes == 0] = 0
    return sizes, A, X


def ici_kendalltau_permdisp(data_matrix, sample_classes, permutations=999, seed=None, strata=None, return_perms=True,
                            global_na=(float("nan"), float("inf"), 0), perspective="global", alternative="two.sided",
                            continuity=False, colnames=None, engine=None):
    """Are the classes of the samples (columns) equally dispersed under ICI-Kendall-tau: PERMDISP (Anderson 2006;
    ``vegan::betadisper(type = "centroid")`` with ``permutest``) on the dissimilarity ``1 - raw`` -- without the S x S
    matrices ``ici_kendalltau`` returns and without a PCoA.  It is the test to run beside ``ici_kendalltau_permanova``
    (Anderson & Walsh 2013): a significant PERMANOVA means "the classes differ in location" only when their
    dispersions are homogeneous.

    ``sample_classes`` gives one label per column (required; the levels are ``ici_kendalltau_class_matrix``'s).  With
    ``d^2 = (1 - raw)^2`` the squared distance of sample i to the centroid of class c, in the full principal-coordinate
    space (real axes minus imaginary axes), is ``(1 / n_c) sum_{j in c} d^2_ij - (1 / n_c^2) sum_{j<k in c} d^2_jk``: it
    needs distances only.  ``distances`` is every sample's distance to its own class centroid (``sqrt(abs(.))``, as
    vegan takes it; ``n_negative`` counts the samples whose squared distance is negative, the sign that the
    dissimilarity is not Euclidean there) -- the multivariate outlier screen --, ``centroid_distance`` [S x C] the
    distance to every class centroid (NA for a class without a sample) and ``nearest_centroid`` the index into
    ``class_levels`` of the class with the smallest squared distance in absolute value, compared exactly, ties to the
    earlier class.  A sample BELONGS to its own class's centroid, as in ``betadisper``; this differs from
    ``ici_kendalltau_class_matrix``, where a sample is not its own partner.  ``statistic`` is the one-way ANOVA F of
    ``distances`` over the classes, ``class_mean_distance`` vegan's "average distance to centroid".

    EXACTNESS.  Every ``(1 - raw)^2`` is PERMANOVA's integer multiple of 2^-50, every squared distance an integer over
    ``n_c^2 2^50``, every distance its correctly rounded square root (``permdisp_distance``); F is computed from those
    doubles as the rationals they are (``permdisp_statistic``).  The result is a pure function of the input and the
    labellings.

    THE PERMUTATION TEST is ``permutest.betadisper``'s: the residuals ``distances - class_mean_distance[class]`` (one
    IEEE subtraction each) are permuted, which is the same as permuting the labels over the fixed residuals.  The
    labellings are ``ici_kendalltau_anosim``'s (``anosim_permutations``): the same ``seed`` and ``strata`` give all three
    tests the same labellings; an integer array [n_perm, S] of class codes is used as given.  ``pvalue`` is
    ``(1 + n_ge) / (1 + n_perm)`` with ``n_ge`` the labellings whose F is defined and ``>=`` the observed F, compared
    exactly; ``n_undefined`` labellings have no F and do not count.  This stage runs on the host.

    EVERY PAIR IS NEEDED.  With a pair whose ``raw`` is NA (``n_na > 0``) no centroid has a meaning: every statistic,
    distance and centroid cell is NA (``nearest_centroid`` -1, ``n_negative`` 0), one warning says so, and the integer
    table is still returned as summed (an NA pair adds 0).  S times the number of classes is at most 2^26.  The other
    arguments are ``ici_kendalltau``'s (column names are required).

    Returns a dict: ``statistic``, ``pvalue``, ``df_among``, ``df_within``, ``ss_among``, ``ss_within``;
    ``n_permutations``, ``n_ge``, ``n_undefined``, ``perm_statistic`` ([n_perm], NA where undefined; only with
    ``return_perms``); ``distances`` [S], ``class_mean_distance``, ``class_size``, ``class_levels``;
    ``centroid_distance`` [S, C], ``nearest_centroid`` [S]; ``n_negative``, ``n_valid``, ``n_na``; ``sums`` (the
    integers: ``q_total``, ``t`` [S, C] and ``class_q`` [C], the within-class sums derived from it); ``sample_id``,
    ``max_taumax`` and ``run_time``.
    """
    data_matrix, names, n_sample, levels, cls, perms = _labellings_input(data_matrix, colnames, sample_classes,
                                                                         permutations, seed, strata)
    n_class, n_perm = len(levels), int(perms.shape[0])
    if n_sample * n_class > _lib.PERMDISP_MAX_CELLS:
        raise ValueError(f"samples x classes must be at most {_lib.PERMDISP_MAX_CELLS}")
    if perms.size and (perms.min() < 0 or perms.max() >= n_class):
        raise ValueError("`permutations` holds a class code outside 0 .. n_class - 1")
    eng = engine or _default_engine()
    if hasattr(eng, "permdisp"):
        (n_pairs, Q, T, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.permdisp(X, cls, n_class, gna, perspective, alternative, continuity, 0))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, True, alternative,
                                               continuity)
        n_pairs, Q, T = _permdisp_numpy(mats5[1], cls, n_class)
    S, n_na = n_sample, int(n_pairs[1])
    sizes, A, X = _permdisp_centroids(T, cls, n_class)
    n_used = int((sizes > 0).sum())
    if n_na > 0:
        warnings.warn(f"PERMDISP needs every pair and {n_na} of them have no raw value: every statistic and distance is "
                      "NA.  `ici_kendalltau_medians` returns `n_valid` per column, which finds the columns to leave out.",
                      RuntimeWarning, stacklevel=2)
        obs = PermdispStatistic((None, None, None, n_used - 1, S - n_used))
        Fs, n_ge, n_undef = [None] * n_perm, 0, n_perm
        z, means, zc = _na_filled(S), _na_filled(n_class), _na_filled((S, n_class))
        nearest, n_negative = np.full(S, -1, dtype=np.int32), 0
    else:
        used = np.flatnonzero(sizes > 0)
        zc = _na_filled((S, n_class))
        for c in used:
            n_c = int(sizes[c])
            zc[:, c] = [permdisp_distance(x, n_c) for x in X[:, c]]
        z = zc[np.arange(S), cls]
        n_negative = int(sum(1 for i in range(S) if X[i, cls[i]] < 0))
        w_sq = math.lcm(*(int(sizes[c]) ** 2 for c in used))
        keys = np.abs(X[:, used]) * np.array([w_sq // int(sizes[c]) ** 2 for c in used], dtype=object)[None, :]
        nearest = used[np.argmin(keys, axis=1)].astype(np.int32)     # (the first of equal keys: the earlier class)
        zi, D = _permdisp_ints(z)
        means = _na_filled(n_class)
        for c in used:
            means[c] = float(Fraction(sum(zi[i] for i in np.flatnonzero(cls == c)), D * int(sizes[c])))
        obs = permdisp_statistic(z, cls, n_class)
        Fs, n_ge, n_undef = _permdisp_permute(z - means[cls], perms, n_class, obs.F)
    return _labellings_result(
        {"statistic": _as_float(obs.F), "pvalue": _na_real() if obs.F is None else float(Fraction(1 + n_ge, 1 + n_perm)),
         "df_among": int(obs.df_among), "df_within": int(obs.df_within), "ss_among": _as_float(obs.ss_among),
         "ss_within": _as_float(obs.ss_within)},
        (n_perm, n_ge, n_undef), {}, Fs if return_perms else None,
        {"distances": z, "class_mean_distance": means, "class_size": sizes}, levels,
        {"centroid_distance": zc, "nearest_centroid": nearest, "n_negative": n_negative, "n_valid": int(n_pairs[0]),
         "n_na": n_na, "sums": {"q_total": int(Q), "t": T, "class_q": np.array(A, dtype=object)}},
        names, max_taumax, t_diff)


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_pcoa: the principal coordinates of the samples under 1 - raw (classical scaling, Gower 1966): the
# largest eigenpairs of the Gower-centred table of PERMANOVA's integers
# --------------------------------------------------------------------------------------------------
def _pcoa_sign(vectors):
    """The sign rule on the columns of `vectors` [S, k], in place: a column's component of largest magnitude is
    positive, the smallest index deciding among equal magnitudes (numpy's argmax takes the first)."""
    for a in range(vectors.shape[1]):
        col = vectors[:, a]
        if col.size and col[int(np.argmax(np.abs(col)))] < 0:
            col *= -1.0
    return vectors


def _pcoa_gower(raw):
    """The integers and the centred table of icikt_pcoa_f64 from a full S x S raw matrix: (n_pairs [2], Q, R [S] of
    Python ints, G [S, S] or None with an NA pair).  q is PERMANOVA's (`_permanova_quantise`), the row sums are taken
    limb by limb in int64, the means are Python's correctly rounded int / int, and
    G = -0.5 * ((q 2^-50 - (m_i + m_j)) + m-bar), one numpy operation -- one rounding -- each."""
    raw = np.asarray(raw, dtype=np.float64)
    S = raw.shape[0]
    iu, ju = np.triu_indices(S, k=1)
    ok = ~np.isnan(raw[iu, ju])
    n_na = int((~ok).sum())
    q = np.zeros((S, S), dtype=np.int64)
    q[iu[ok], ju[ok]] = _permanova_quantise(raw[iu[ok], ju[ok]])
    q = q + q.T
    R = _lib._limbs_to_ints((q & 0xFFFFFFFF).sum(axis=1), (q >> 32).sum(axis=1))
    T = sum(int(r) for r in R)
    n_pairs = np.array([int(ok.sum()), n_na], dtype=np.int64)
    if n_na > 0:
        return n_pairs, T // 2, R, None
    m = np.array([int(r) / (S << PERMANOVA_FRAC_BITS) for r in R], dtype=np.float64)
    grand = T / ((S * S) << PERMANOVA_FRAC_BITS)
    e = np.ldexp(q.astype(np.float64), -PERMANOVA_FRAC_BITS)
    G = -0.5 * ((e - (m[:, None] + m[None, :])) + grand)
    return n_pairs, T // 2, R, G


def _pcoa_numpy(raw, k):
    """icikt_pcoa_f64's result from a full S x S raw matrix with numpy.linalg.eigh, for engines without a pcoa method
    (the CPU tests' checker engines): Context.pcoa's tuple without max_taumax and reason_counts.  The whole spectrum is
    computed, so n_basis is S, n_apply 0 and the call has always converged."""
    n_pairs, Q, R, G = _pcoa_gower(raw)
    S = len(R)
    if G is None:
        return (n_pairs, Q, R, _na_filled(k), _na_filled((S, k)), _na_filled(k), _na_real(), _na_real(), 0, 0, False, None)
    w, V = np.linalg.eigh(G)
    lam = w[::-1][:k].copy()
    vec = _pcoa_sign(np.ascontiguousarray(V[:, ::-1][:, :k]))
    res = np.linalg.norm(G @ vec - vec * lam, axis=0)
    return (n_pairs, Q, R, lam, vec, res, float(np.linalg.norm(G)), float(w[0]), S, 0, True, G)


def ici_kendalltau_pcoa(data_matrix, k=10, tol=1e-8, max_basis=None, seed=0, return_gower=False,
                        global_na=(float("nan"), float("inf"), 0), perspective="global", alternative="two.sided",
                        continuity=False, colnames=None, engine=None):
    """The ordination of the samples (columns) under ICI-Kendall-tau: principal coordinates analysis (classical
    scaling, Gower 1966; ``vegan::wcmdscale``, ``skbio.stats.ordination.pcoa``) on the dissimilarity ``1 - raw``, with
    the share of inertia per axis -- without the S x S matrices ``ici_kendalltau`` returns.  It decomposes exactly the
    inertia ``ici_kendalltau_permanova`` partitions (``total_inertia`` is its ``ss_total``) and draws the space
    ``ici_kendalltau_permdisp`` measures its distances in.

    The rule.  Every ``(1 - raw)^2`` is PERMANOVA's integer multiple of 2^-50; the row and grand means of those squared
    dissimilarities are correctly rounded doubles of integer ratios; ``G = -0.5 (d^2 - row mean - column mean + grand
    mean)``, in a fixed order of four double operations, is the Gower-centred table, symmetric to the bit.  The result
    is the ``k`` algebraically largest eigenvalues of G, descending, with orthonormal eigenvectors: ``coordinates[:, a] =
    vectors[:, a] * sqrt(eigenvalues[a])`` where the eigenvalue is positive, else 0; ``proportion = eigenvalues /
    total_inertia`` with ``total_inertia = trace(G)``, from the integers; ``n_positive`` counts the positive eigenvalues
    among the k.  A vector's component of largest magnitude is positive (the smallest index decides among equal
    magnitudes), so an axis does not flip between runs.

    THE SOLVER is a block Krylov iteration with full reorthogonalisation and Rayleigh-Ritz on the device, from a start
    block of ``numpy.random.default_rng(seed)`` normals: it stops when every residual ``|G y - lambda y|`` is within
    ``tol |G|_F``, or when the basis holds ``max_basis`` columns (default ``min(S, max(8 k, 128))``, at most 512) -- then
    the best pairs so far are returned with ``converged = False``, ``residuals`` as they are and one warning.  With
    ``max_basis = S`` the basis spans the space and the call always converges.  Every floating-point sum on the device
    has a fixed order: the same input and seed give the same bits.  ``min_ritz``, the smallest Ritz value of the last
    projected problem, estimates (from above) the most negative eigenvalue of G: how far the dissimilarity is from
    Euclidean.

    EVERY PAIR IS NEEDED.  With a pair whose ``raw`` is NA (``n_na > 0``) the centring has no meaning: every double is
    NA, one warning says so, and the integers are still returned.  ``1 <= k <= min(S - 1, 64)``; S is at least 2 and at
    most 65 535.  The other arguments are ``ici_kendalltau``'s (column names are required).

    Returns a dict: ``coordinates`` [S, k], ``eigenvalues`` [k], ``proportion`` [k], ``vectors`` [S, k],
    ``total_inertia``, ``n_positive``; ``residuals`` [k], ``frobenius``, ``min_ritz``, ``n_basis``, ``n_apply``,
    ``converged``; ``n_valid``, ``n_na``; ``sums`` (the integers: ``q_total`` and ``row_q`` [S]); ``gower`` ([S, S], only
    with ``return_gower``); ``sample_id``, ``max_taumax`` and ``run_time``.
    """
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    if n_sample < 2:
        raise ValueError("ici_kendalltau_pcoa needs at least 2 samples")
    k = _int_arg(k, 1, min(n_sample - 1, _lib.PCOA_MAX_K), "`k` must be an integer in 1 .. min(S - 1, 64)")
    if isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (int, float, np.integer, np.floating)) \
            or not (float(tol) > 0.0 and math.isfinite(float(tol))):
        raise ValueError("`tol` must be a positive number")
    if max_basis is not None:
        max_basis = _int_arg(max_basis, k, 2 ** 31 - 1, "`max_basis` must be None or an integer that is at least k")
    eng = engine or _default_engine()
    if hasattr(eng, "pcoa"):
        (n_pairs, Q, R, lam, vec, res, frob, min_ritz, n_basis, n_apply, converged, G, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.pcoa(X, k, float(tol), max_basis, seed, bool(return_gower), gna, perspective, alternative,
                                    continuity, 0))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, True, alternative,
                                               continuity)
        n_pairs, Q, R, lam, vec, res, frob, min_ritz, n_basis, n_apply, converged, G = _pcoa_numpy(mats5[1], k)
    S, n_na = n_sample, int(n_pairs[1])
    if n_na > 0:
        warnings.warn(f"PCoA needs every pair and {n_na} of them have no raw value: every eigenvalue and coordinate is "
                      "NA.  `ici_kendalltau_medians` returns `n_valid` per column, which finds the columns to leave out.",
                      RuntimeWarning, stacklevel=2)
        total, coords, prop, n_positive = _na_real(), _na_filled((S, k)), _na_filled(k), 0
        G = _na_filled((S, S)) if return_gower else None
    else:
        if not converged:
            warnings.warn(f"PCoA has not converged within {int(n_basis)} basis columns: the largest residual is "
                          f"{float(np.max(res)):.3g} against tol |G|_F = {float(tol) * frob:.3g}.  Raise `max_basis` (at "
                          "most 512, or S), or loosen `tol`.", RuntimeWarning, stacklevel=2)
        total = float(Fraction(int(Q), S << PERMANOVA_FRAC_BITS))
        pos = lam > 0
        coords = np.where(pos[None, :], vec * np.sqrt(np.where(pos, lam, 0.0))[None, :], 0.0)
        prop = lam / total if total != 0 else _na_filled(k)
        n_positive = int(pos.sum())
    out = {"coordinates": coords, "eigenvalues": lam, "proportion": prop, "vectors": vec, "total_inertia": total,
           "n_positive": n_positive, "residuals": res, "frobenius": frob, "min_ritz": min_ritz, "n_basis": int(n_basis),
           "n_apply": int(n_apply), "converged": bool(converged), "n_valid": int(n_pairs[0]), "n_na": n_na,
           "sums": {"q_total": int(Q), "row_q": R}}
    if return_gower:
        out["gower"] = G
    out.update({"sample_id": np.asarray(list(names), dtype=object), "max_taumax": max_taumax, "run_time": t_diff})
    return out


# --------------------------------------------------------------------------------------------------
# ici_kendalltau_mantel: the Mantel test (Mantel 1967; vegan::mantel, skbio.stats.distance.mantel) of the dissimilarity
# 1 - raw against another matrix of the same samples, in integers (csrc/icikt_mantel.h)
# --------------------------------------------------------------------------------------------------
MANTEL_X_FRAC_BITS = 30   # mantel::X_FRAC_BITS: xv = (1 - raw) 2^30, rounded half to even
MANTEL_Y_BITS = 31        # mantel::Y_BITS: yv = (y - lo) 2^(31 - e), (m, e) = frexp(hi - lo)


def mantel_permutations(S, permutations=999, seed=None, strata=None):
    """The permutations ``ici_kendalltau_mantel`` compares with, [n_perm, S] int32 sample indices:
    ``anosim_permutations(numpy.arange(S), permutations, seed, strata)``.  Permutation t sends sample s to
    ``perms[t, s]``, and ``codes[perms[t]]`` is the labelling ``ici_kendalltau_anosim``, ``ici_kendalltau_permanova``
    and ``ici_kendalltau_permdisp`` draw for the same ``seed`` and ``strata``.  An integer array [n_perm, S] is returned
    as given (as int32)."""
    return anosim_permutations(np.arange(int(S), dtype=np.int32), permutations, seed, strata)


def _sqrt_fraction(A, B):
    """The correctly rounded double of sqrt(A / B) for integers A >= 0 and B > 0 (``permdisp_distance``'s recipe): e is
    chosen so that N = floor((A / B) 4^e) has 127 or 128 bits and m is its integer square root (64 bits); m' = 2 m when
    (A / B) 4^e is the integer m^2 and 2 m + 1 otherwise: the sticky bit makes the one conversion of m' / 2^(e + 1)
    round correctly."""
    A, B = int(A), int(B)
    if A == 0:
        return 0.0
    e = (127 - (A.bit_length() - B.bit_length())) // 2
    while True:
        num, d = (A << (2 * e), B) if e >= 0 else (A, B << (-2 * e))
        N, rest = divmod(num, d)
        bits_n = N.bit_length()
        if bits_n < 127:
            e += 1
        elif bits_n > 128:
            e -= 1
        else:
            break
    m = math.isqrt(N)
    m2 = 2 * m if (rest == 0 and m * m == N) else 2 * m + 1
    return float(Fraction(m2, 1 << (e + 1)) if e + 1 >= 0 else Fraction(m2 << -(e + 1)))


def mantel_statistic(P, T, sx, sxx, sy, syy):
    """The Mantel statistic r of one permutation as a correctly rounded double, from the integers of icikt_mantel_f64:
    P pairs, T = sum x y, and the moments sum x, sum x^2, sum y, sum y^2.  With num = P T - sx sy and
    den = (P sxx - sx^2)(P syy - sy^2), r = num / sqrt(den): the sign of num times the correctly rounded root of
    num^2 / den.  None when a factor of den is 0 (x or y is constant, or P = 0): r is undefined."""
    P, T, sx, sxx, sy, syy = (int(v) for v in (P, T, sx, sxx, sy, syy))
    vx, vy = P * sxx - sx * sx, P * syy - sy * sy
    if P <= 0 or vx <= 0 or vy <= 0:
        return None
    num = P * T - sx * sy
    root = _sqrt_fraction(num * num, vx * vy)
    return -root if num < 0 else root


def _mantel_rank2(values, descending):
    """The doubled average rank of every value among all of them, -0 as +0: ascending lo + hi + 1 (lo the values below,
    hi those at or below), descending 2 M - lo - hi + 1, as int64."""
    v = np.asarray(values, dtype=np.float64) + 0.0
    asc = np.sort(v)
    lo = np.searchsorted(asc, v, "left").astype(np.int64)
    hi = np.searchsorted(asc, v, "right").astype(np.int64)
    return 2 * v.shape[0] - lo - hi + 1 if descending else lo + hi + 1


def _mantel_quantise_x(raw):
    """mantel::quantise_x (csrc/icikt_mantel.h) on an array of raw values without NaN, as int64: -0 is +0, d = 1.0 - raw
    in double, xv = rint(ldexp(d, 30))."""
    return np.rint(np.ldexp(1.0 - (np.asarray(raw, dtype=np.float64) + 0.0), MANTEL_X_FRAC_BITS)).astype(np.int64)


def _mantel_quantise_y(y):
    """mantel::quantise_y on the finite doubles y, as int64: lo and hi the smallest and largest, span = hi - lo one
    double operation, (m, e) = frexp(span), yv = rint(ldexp(y - lo, 31 - e)).  A span that is not finite is refused."""
    y = np.asarray(y, dtype=np.float64)
    if y.size == 0:
        return np.zeros(0, dtype=np.int64)
    lo, hi = y.min(), y.max()
    with np.errstate(over="ignore"):
        span = hi - lo
    if not np.isfinite(span):
        raise ValueError("the span of `other` (its largest minus its smallest value) is not finite")
    e = int(np.frexp(span)[1])
    return np.rint(np.ldexp(y - lo, MANTEL_Y_BITS - e)).astype(np.int64)


def _mantel_dot(x, y):
    """sum x y of two int64 arrays of values below 2^32, as a Python int: the four products of the 16-bit halves are
    each below 2^32, and a sum of fewer than 2^31 of them stays in int64."""
    xl, xh, yl, yh = x & 0xFFFF, x >> 16, y & 0xFFFF, y >> 16
    ll, lh, hl, hh = (int(np.dot(a, b)) for a, b in ((xl, yl), (xl, yh), (xh, yl), (xh, yh)))
    return ll + ((lh + hl) << 16) + (hh << 32)


def _mantel_numpy(raw, other, method, perms):
    """The integers of icikt_mantel_f64 from a full S x S raw matrix and the condensed `other`, for engines without a
    mantel method (the CPU tests' checker engines): (n_pairs [2], T [1 + n_perm] of Python ints, (sx, sxx, sy, syy),
    n_ge, n_le)."""
    raw = np.asarray(raw, dtype=np.float64)
    S = raw.shape[0]
    iu, ju = np.triu_indices(S, k=1)
    v = raw[iu, ju]
    n_na = int(np.isnan(v).sum())
    perms = np.asarray(perms, dtype=np.int64).reshape(-1, S)
    T = np.zeros(1 + perms.shape[0], dtype=object)
    n_pairs = np.array([v.shape[0] - n_na, n_na], dtype=np.int64)
    if n_na > 0 or v.shape[0] == 0:
        n_cmp = 0 if n_na > 0 else perms.shape[0]
        return n_pairs, T, (0, 0, 0, 0), n_cmp, n_cmp
    if method == "spearman":
        xv, yv = _mantel_rank2(v, True), _mantel_rank2(other, False)
    else:
        xv, yv = _mantel_quantise_x(v), _mantel_quantise_y(other)
    table = np.zeros((S, S), dtype=np.int64)
    table[iu, ju] = yv
    table[ju, iu] = yv
    for t, pi in enumerate(np.vstack([np.arange(S, dtype=np.int64)[None, :], perms])):
        T[t] = _mantel_dot(xv, table[pi[iu], pi[ju]])
    n_ge = sum(1 for t in T[1:] if t >= T[0])
    n_le = sum(1 for t in T[1:] if t <= T[0])
    return n_pairs, T, (int(xv.sum()), _mantel_dot(xv, xv), int(yv.sum()), _mantel_dot(yv, yv)), n_ge, n_le


def _mantel_other(other, S):
    """`other` of ici_kendalltau_mantel as the condensed float64 vector of its P pairs in combn order."""
    if _lib.is_sparse(other):
        other = other.toarray()
    a = np.asarray(other)
    if a.dtype == object or not (np.issubdtype(a.dtype, np.number) or a.dtype == np.bool_):
        raise ValueError("`other` must be numeric")
    a = np.asarray(a, dtype=np.float64)
    P = S * (S - 1) // 2
    if a.ndim == 2 and a.shape == (S, S):
        iu, ju = np.triu_indices(S, k=1)
        upper, lower = a[iu, ju], a[ju, iu]
        both_nan = np.isnan(upper) & np.isnan(lower)
        differ = np.flatnonzero((upper != lower) & ~both_nan)
        if differ.size:
            i, j = int(iu[differ[0]]), int(ju[differ[0]])
            raise ValueError(f"`other` must be exactly symmetric: other[{i}, {j}] = {float(a[i, j])!r} but "
                             f"other[{j}, {i}] = {float(a[j, i])!r}")
        vec = np.ascontiguousarray(upper)
    elif a.ndim == 1 and a.shape[0] == P:
        vec = np.ascontiguousarray(a)
    else:
        raise ValueError(f"`other` must be an S x S matrix or a condensed vector of length S (S - 1) / 2 "
                         f"(S = {S}: {P}), not of shape {a.shape}")
    bad = np.flatnonzero(~np.isfinite(vec))
    if bad.size:
        iu, ju = np.triu_indices(S, k=1)
        raise ValueError(f"`other` must be finite: the value of pair ({int(iu[bad[0]])}, {int(ju[bad[0]])}) is "
                         f"{float(vec[bad[0]])!r}")
    return vec


def ici_kendalltau_mantel(data_matrix, other, method="pearson", permutations=999, seed=None, strata=None,
                          return_perms=True, global_na=(float("nan"), float("inf"), 0), perspective="global",
                          alternative="two.sided", continuity=False, colnames=None, engine=None):
    """Does the structure of the ICI-Kendall-tau correlations of the samples (columns) agree with ANOTHER matrix of the
    same samples -- another omics layer, run order or collection time as ``|t_i - t_j|``, geographic distance, the
    distances of ``cor_fast``, a 0/1 design matrix: the Mantel test (Mantel 1967; ``vegan::mantel``,
    ``skbio.stats.distance.mantel``) of the dissimilarity ``1 - raw`` against ``other``, with its permutation test --
    without the S x S matrices ``ici_kendalltau`` returns.

    ``other`` is an S x S array (exactly symmetric; its diagonal is ignored) or a condensed vector with one value per
    pair i < j (``scipy.spatial.distance.squareform`` order), every value finite.  ``statistic`` is the correlation r
    of the two vectors of P = S (S - 1) / 2 pairs: Pearson's (``method="pearson"``, the default, as in vegan) or
    Spearman's (``method="spearman"``: both vectors are replaced by their average ranks).  r is NA when either vector
    is constant.

    EXACTNESS.  Both vectors become integers below 2^32 by one fixed rule -- for spearman the doubled average ranks
    (-0 equals +0), for pearson ``rint((1 - raw) 2^30)`` and ``rint((y - min) 2^(31 - e))`` with ``(m, e) =
    frexp(max - min)``, which moves each value by at most 2^-31 of its range -- and everything after that is integer
    arithmetic: T(pi) = sum x_ij y_pi(i)pi(j), the moments, and the comparison of T(pi) with the observed T.  The
    result is a pure function of the input, ``other`` and the permutations; a 0/1 design matrix gives many exactly
    equal T, and they compare as equal.  ``statistic`` and ``perm_statistic`` come from the integers by one correctly
    rounded square root (``mantel_statistic``).

    EVERY PAIR IS NEEDED.  With a pair whose ``raw`` is NA (``n_na > 0``) nothing is imputed and no pair is dropped:
    every double of the result is NA, and one warning says so.  ``ici_kendalltau_medians`` gives ``n_valid`` per column,
    which finds the columns to leave out.

    THE PERMUTATIONS permute the samples of ``other`` (rows and columns together); they are fixed by (S, ``seed``,
    ``strata``): ``mantel_permutations`` is the rule, and ``codes[perm_t]`` is the labelling ``ici_kendalltau_anosim``
    draws for the same seed.  ``permutations`` is their number (999, at most 1 000 000) or an integer array [n_perm, S]
    whose rows are permutations of 0 .. S - 1, used as given.  ``pvalue`` is ``(1 + n_ge) / (1 + n_perm)`` with
    ``n_ge`` the permutations whose T is ``>=`` the observed T (vegan's one-sided test for a positive association);
    ``n_le`` counts ``<=`` for the other side.  On the HIP engine everything up to the integers runs on the device
    (icikt_mantel_f64); a matrix has at most 65 535 samples and the table of ``other`` takes 4 S^2 bytes there.  The
    other arguments are ``ici_kendalltau``'s (column names are required).

    Returns a dict: ``statistic``, ``pvalue``, ``n_permutations``, ``n_ge``, ``n_le``, ``n_valid``, ``n_na``,
    ``perm_statistic`` ([n_perm]; only with ``return_perms``), ``method``, ``sums`` (the integers: ``T`` [1 + n_perm],
    index 0 the observed one, ``sx``, ``sxx``, ``sy``, ``syy``), ``sample_id``, ``max_taumax`` and ``run_time``.
    """
    if method not in _lib.MANTEL:
        raise ValueError('`method` must be "pearson" or "spearman"')
    data_matrix, names, n_sample = _select_input(data_matrix, colnames)
    _need_pairs(n_sample)
    S = n_sample
    vec = _mantel_other(other, S)
    if method == "pearson":
        _mantel_quantise_y(np.array([vec.min(), vec.max()]))   # (refuses a span that is not finite)
    perms = mantel_permutations(S, permutations, seed, strata)
    if perms.size and not np.array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(S, dtype=np.int32), perms.shape)):
        raise ValueError("every row of `permutations` must be a permutation of 0 .. S - 1")
    n_perm = int(perms.shape[0])
    eng = engine or _default_engine()
    if hasattr(eng, "mantel"):
        (n_pairs, T, mom, n_ge, n_le, max_taumax), t_diff = _on_device(
            eng, data_matrix, global_na,
            lambda X, gna: eng.mantel(X, vec, method, perms if n_perm else None, gna, perspective, alternative,
                                      continuity, 0))
    else:
        mats5, t_diff, max_taumax = _from_full(eng, data_matrix, names, global_na, perspective, True, alternative,
                                               continuity)
        n_pairs, T, mom, n_ge, n_le = _mantel_numpy(mats5[1], vec, method, perms)
    P, n_na = S * (S - 1) // 2, int(n_pairs[1])
    if n_na > 0:
        warnings.warn(f"The Mantel test needs every pair and {n_na} of them have no raw value: every statistic is NA.  "
                      "`ici_kendalltau_medians` returns `n_valid` per column, which finds the columns to leave out.",
                      RuntimeWarning, stacklevel=2)
        obs, stats = None, [None] * n_perm
    else:
        obs = mantel_statistic(P, T[0], *mom)
        stats = [mantel_statistic(P, t, *mom) for t in T[1:]] if return_perms else None
    res = {"statistic": _as_float(obs), "pvalue": _na_real() if obs is None else float(Fraction(1 + int(n_ge), 1 + n_perm)),
           "n_permutations": n_perm, "n_ge": int(n_ge), "n_le": int(n_le), "n_valid": int(n_pairs[0]), "n_na": n_na}
    if return_perms:
        res["perm_statistic"] = np.array([_as_float(f) for f in stats], dtype=np.float64)
    res.update({"method": method, "sums": {"T": T, "sx": int(mom[0]), "sxx": int(mom[1]), "sy": int(mom[2]), "syy": int(mom[3])},
                "sample_id": list(names), "max_taumax": max_taumax, "run_time": t_diff})
    return res


# --------------------------------------------------------------------------------------------------
# pairwise_completeness (R/kendalltau.R:563-629)
# --------------------------------------------------------------------------------------------------
def pairwise_completeness(data_matrix, global_na=(float("nan"), float("inf"), 0), include_only=None,
                          return_matrix=True, colnames=None, engine=None):
    """Pairwise completeness of the samples (R/kendalltau.R:563-629).  A sparse ``data_matrix`` stays sparse on a HIP
    engine: the rule of ``global_na`` is applied to its stored values and to the value of its absent cells (0), O(nnz)
    on the host, and the CSC arrays go to the device (icikt_missingness_csc); any other engine gets ``toarray()``."""
    eng = engine or _default_engine()
    data_matrix, names = _as_matrix(data_matrix, colnames, "data_matrix", keep_sparse=isinstance(eng, HipEngine))
    _dist, _rank, world = _dist_info()
    pi, pj, core = setup_comparisons(names, include_only, diag_good=False, ncore=world)
    n_feat = data_matrix.shape[0]
    if _lib.is_sparse(data_matrix):
        s = _lib.csc_view(data_matrix)
        stored = np.where(setup_missing_matrix(np.asarray(s.data, dtype=np.float64), global_na), np.nan, 0.0)
        absent = np.nan if bool(setup_missing_matrix(np.zeros(1), global_na)[0]) else 0.0
        masked = _lib.CscView(stored, s.indices, s.indptr, s.shape, np.array([absent]), True)
    else:
        exclude_loc = setup_missing_matrix(data_matrix, global_na)
        masked = np.asfortranarray(np.where(exclude_loc, np.nan, 0.0))
    missingness = eng.missingness(masked, pi, pj).astype(np.float64)
    completeness = 1 - (missingness / n_feat)
    if return_matrix:
        m = np.zeros((len(names), len(names)))
        m[pi, pj] = completeness
        m[pj, pi] = completeness
        return _named_matrix(m, names)
    names_arr = np.asarray(names, dtype=object)
    cols = {"s1": names_arr[pi], "s2": names_arr[pj], "core": core.astype(np.float64), "missingness": missingness,
            "completeness": completeness}
    return pd.DataFrame(cols) if pd is not None else cols


# --------------------------------------------------------------------------------------------------
# kt_fast (R/kendalltau.R:448-545) and kt_split (:310-354) -- SURVEY.md section 8(f) row 3
# --------------------------------------------------------------------------------------------------
_KT_USE = ("all.obs", "complete.obs", "pairwise.complete.obs", "everything", "na.or.complete")


def _match_use(use: str) -> str:
    """R's match.arg(): exact or unique partial match."""
    hits = [u for u in _KT_USE if u == use] or [u for u in _KT_USE if u.startswith(use)]
    if len(hits) != 1:
        raise ValueError("'arg' should be one of " + ", ".join(f"'{u}'" for u in _KT_USE))
    return hits[0]


def kt_fast(x, y=None, use="everything", alternative="two.sided", continuity=False, return_matrix=True,
            colnames=None, engine=None, max_pair_chunk=4096):
    """Kendall tau-b with stats::cor-like NA policies over the ici_kt kernel (R/kendalltau.R:448-545).

    As in the reference, ``alternative`` and ``continuity`` are accepted but NOT forwarded (kt_split calls
    ici_kt with its defaults, :342), and self comparisons are part of the result.  ``use``:
    "everything"/"all.obs": any NA anywhere in ``x`` -> every entry NA; "complete.obs": rows with an NA in
    any column are dropped first; "pairwise.complete.obs": per pair, rows with an NA in either vector are
    dropped.  The last one runs on the GPU as ici_kt(..., perspective = "local") of the two vectors with both
    entries of such rows set missing -- identical to dropping the rows, since "local" removes rows missing in
    both (src/kendallc.cpp:180-185) and nothing missing remains; the HIP engine masks, sorts and counts every
    pair on the device (icikt_pairs_complete_f64), other engines get the masked vectors from the host -- as does the
    HIP engine for columns of more than 65 535 rows, which that entry does not take.
    """
    if _lib.is_sparse(x):   # zero is a value here, not a missing cell: the dense matrix is what is meant
        x = _densify(x)
    na_method = _match_use(use)
    if na_method == "na.or.complete":
        raise ValueError("'na.or.complete' is not a supported value for `use`. "
                         "Please use one of all.obs complete.obs pairwise.complete everthing.")  # R/utils.R:86-90 (sic)
    if y is None:
        if not (pd is not None and isinstance(x, pd.DataFrame)) and np.ndim(x) < 2:
            raise ValueError("`x` and `y` should both be provided as vectors, or `x` should be matrix-like.")
        X, names = _as_matrix(x, colnames, "x", keep_dtype=True)
    else:
        if np.ndim(x) > 1 or np.ndim(y) > 1:
            raise ValueError("Both `x` and `y` must be vectors.")
        X = np.column_stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
        names = list(colnames) if colnames is not None else ["x", "y"]
    eng = engine or _default_engine()
    _dist, _rank, world = _dist_info()
    pi, pj, core = setup_comparisons(names, None, diag_good=False, ncore=world)
    P = len(pi)
    tau = np.full(P, np.nan)
    pvalue = np.full(P, np.nan)
    na_vals = np.isnan(X)
    t_diff = 0.0
    do_computation = True
    if na_method in ("everything", "all.obs") and na_vals.any():
        do_computation = False
    if na_method == "complete.obs":
        keep = ~na_vals.any(axis=1)
        if keep.sum() == 0:
            do_computation = False
        else:
            X = np.asarray(X, dtype=np.float64)[keep]
    if do_computation:
        t1 = time.perf_counter()
        if na_method == "pairwise.complete.obs" and np.isnan(X).any() and hasattr(eng, "pairs_complete") and \
                X.shape[0] <= _lib.MAX_FEATURES:
            # masking, per-pair sorts and counting on the device (icikt_pairs_complete_in: no path for wide columns,
            # which take the host-masked loop below through eng.pairs)
            out, rsn = eng.pairs_complete(_for_engine(X, eng), pi, pj)
            for r in rsn[rsn > 1]:
                _warn_reason(r)
            tau, pvalue = out[:, 0].copy(), out[:, 1].copy()
        elif na_method == "pairwise.complete.obs" and np.isnan(X).any():
            X = np.asarray(X, dtype=np.float64)
            na = np.isnan(X)
            for b in range(0, P, max_pair_chunk):
                sl = slice(b, min(P, b + max_pair_chunk))
                m = sl.stop - sl.start
                either = na[:, pi[sl]] | na[:, pj[sl]]
                Xp = np.empty((X.shape[0], 2 * m), dtype=np.float64, order="F")
                Xp[:, 0::2] = np.where(either, np.nan, X[:, pi[sl]])
                Xp[:, 1::2] = np.where(either, np.nan, X[:, pj[sl]])
                idx = np.arange(m, dtype=np.int32)
                out, rsn = eng.pairs(Xp, 2 * idx, 2 * idx + 1, "local", "two.sided", False)
                for r in rsn[rsn > 1]:
                    _warn_reason(r)
                tau[sl], pvalue[sl] = out[:, 0], out[:, 1]
        else:
            out, rsn = eng.pairs(_for_engine(X, eng), pi, pj, "local", "two.sided", False)
            for r in rsn[rsn > 1]:
                _warn_reason(r)
            tau, pvalue = out[:, 0].copy(), out[:, 1].copy()
        t_diff = time.perf_counter() - t1
    if return_matrix:
        S = len(names)
        tm, pm = np.zeros((S, S)), np.zeros((S, S))
        tm[pi, pj] = tau
        tm[pj, pi] = tau
        pm[pi, pj] = pvalue
        pm[pj, pi] = pvalue
        return {"tau": _named_matrix(tm, names), "pvalue": _named_matrix(pm, names), "run_time": t_diff}
    names_arr = np.asarray(names, dtype=object)
    cols = {"s1": names_arr[pi], "s2": names_arr[pj], "core": core.astype(np.float64), "tau": tau, "pvalue": pvalue}
    return {"tau": pd.DataFrame(cols) if pd is not None else cols, "run_time": t_diff}


# --------------------------------------------------------------------------------------------------
# cor_fast (R/other_correlations.R) -- DESIGN.md section 9
# --------------------------------------------------------------------------------------------------
_COR_TIES_WARNING = "Cannot compute exact p-value with ties"


def _lgammacor(x):
    r = 1.0 / x
    r2 = r * r
    return r * (1 / 12 + r2 * (-1 / 360 + r2 * (1 / 1260 + r2 * (-1 / 1680 + r2 * (1 / 1188 + r2 * (-691 / 360360))))))


def _lbeta(a, b):
    """log B(a, b) as R's lbeta computes it (no cancellation of lgamma differences at large arguments)."""
    p, q = min(a, b), max(a, b)
    if p >= 10:
        corr = _lgammacor(p) + _lgammacor(q) - _lgammacor(p + q)
        return -0.5 * math.log(q) + 0.918938533204672741780329736406 + corr + (p - 0.5) * math.log(p / (p + q)) + \
            q * math.log1p(-p / (p + q))
    if q >= 10:
        corr = _lgammacor(q) - _lgammacor(p + q)
        return math.lgamma(p) + corr + p - p * math.log(p + q) + (q - 0.5) * math.log1p(-p / (p + q))
    return math.lgamma(p) + math.lgamma(q) - math.lgamma(p + q)


def _incbeta_cf(a, b, x, y, front=None):
    """The continued fraction of I_x(a, b) times its front factor x^a y^b / (a B(a, b)) (computed here unless given)."""
    tiny, eps = 1e-300, 1e-16
    if front is None:
        front = math.exp(a * math.log(x) + b * math.log(y) - _lbeta(a, b)) / a
    d = 1.0 - (a + b) * x / (a + 1.0)
    d = 1.0 / (tiny if abs(d) < tiny else d)
    c, f = 1.0, d
    for m in range(1, 200000):
        for num in (m * (b - m) * x / ((a + 2 * m - 1) * (a + 2 * m)),
                    -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1))):
            d = 1.0 + num * d
            d = 1.0 / (tiny if abs(d) < tiny else d)
            c = 1.0 + num / c
            c = tiny if abs(c) < tiny else c
            f *= d * c
        if abs(d * c - 1.0) < eps:
            break
    return front * f


def _incbeta(a, b, x, y):
    """Regularized incomplete beta I_x(a, b); y = 1 - x, given separately."""
    if x <= 0:
        return 0.0
    if y <= 0:
        return 1.0
    if x > (a + 1) / (a + b + 2):
        return 1.0 - _incbeta_cf(b, a, y, x)
    return _incbeta_cf(a, b, x, y)


def _t_tail(t, df):
    """P(T > |t|), Student's t with df degrees of freedom."""
    if math.isinf(t):
        return 0.0
    t2 = t * t
    return 0.5 * _incbeta(0.5 * df, 0.5, df / (df + t2), t2 / (df + t2))


def _pt(t, df, lower):
    if math.isnan(t) or not df > 0:
        return math.nan
    tail = _t_tail(t, df)
    return tail if lower == (t < 0) else 1.0 - tail


_PRHO_UPPER: dict = {}


def _prho_upper(n):
    """upper[k] = permutations of n rows whose S = sum (i - perm(i))^2 is >= 2 k (n <= 9)."""
    if n not in _PRHO_UPPER:
        import itertools
        base = np.arange(n)
        counts = np.zeros((n ** 3 - n) // 6 + 1, dtype=np.int64)
        for perm in itertools.permutations(range(n)):
            counts[int(((base - np.asarray(perm)) ** 2).sum()) // 2] += 1
        _PRHO_UPPER[n] = np.cumsum(counts[::-1])[::-1]
    return _PRHO_UPPER[n]


def _prho(is_, n, lower):
    """AS 89 (R's prho): P[S >= is] (lower = False) or P[S < is] (lower = True) for n untied rows."""
    pv = 0.0 if lower else 1.0
    if n <= 1 or is_ <= 0:
        return pv
    if is_ > n * (n * n - 1) / 3:
        return 1.0 - pv
    if n <= 9:
        fact = math.factorial(n)
        ifr = float(_prho_upper(n)[int(math.ceil(is_ / 2))])
        return (fact - ifr if lower else ifr) / fact
    b = 1.0 / n
    x = (6.0 * (is_ - 1) * b / (n * n - 1) - 1) * math.sqrt(1 / b - 1)
    y = x * x
    u = x * b * (0.2274 + b * (0.2531 + 0.1745 * b) + y * (-0.0758 + b * (0.1033 + 0.3932 * b) - y * b * (
        0.0879 + 0.0151 * b - y * (0.0072 - 0.0831 * b + y * b * (0.0131 - 4.6e-4 * y)))))
    y = u / math.exp(y / 2)
    up = 0.5 * math.erfc(x / math.sqrt(2))
    pv = (1.0 - up) - y if lower else y + up
    return min(1.0, max(0.0, pv))


def _pspearman(q, n, lower, exact, continuity):
    if n <= 1290 and exact:
        return _prho(round(q) + 2 * lower, n, lower)
    den = n * (n * n - 1) / 6
    r = 1 - q / den
    if continuity:
        r -= math.copysign(1.0, r) / den if r != 0 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        t = float(np.float64(r) / np.sqrt(np.float64((1 - r * r) / (n - 2)))) if n > 2 else math.nan
    return _pt(t, n - 2, not lower)


def cor_test_pvalue(rho, n, method, alternative="two.sided", continuity=False, ties=False):
    """stats::cor.test.default's p-value of an estimate rho over n rows: the same formulas the
    device epilogue (icikt_cor.hip, k_cor_epilogue) runs."""
    if math.isnan(rho):
        return math.nan
    if method == "pearson":
        df = n - 2
        # 1 - rho^2 as (1 - rho)(1 + rho): a rounded rho * rho costs 1 - rho^2 up to 3.7e-9 relative (at 1 - |rho| near
        # 2^-27) and p df/2 times that.  The device's 1 - rho * rho is one fma, which loses nothing either.
        with np.errstate(divide="ignore", invalid="ignore"):
            t = float(np.sqrt(np.float64(df)) * rho / np.sqrt(np.float64((1 - rho) * (1 + rho))))
        if alternative == "two.sided":
            return 2.0 * _t_tail(t, df)
        return _pt(t, df, alternative == "less")
    exact = n < 1290 and not ties
    q = (n ** 3 - n) * (1 - rho) / 6
    if alternative == "two.sided":
        p = _pspearman(q, n, not (q > (n ** 3 - n) / 6), exact, continuity)
        return min(2 * p, 1.0)
    return _pspearman(q, n, alternative == "greater", exact, continuity)


def _rank2(v):
    """2 * rank(v, ties.method = "average") (integers), and whether v has ties."""
    order = np.argsort(v, kind="stable")
    sv = v[order]
    starts = np.r_[True, sv[1:] != sv[:-1]]
    gid = np.cumsum(starts) - 1
    first = np.flatnonzero(starts)
    ends = np.r_[first[1:], len(v)]
    r = np.empty(len(v), dtype=np.int64)
    r[order] = first[gid] + ends[gid] + 1
    return r, bool(len(first) < len(v))


def _pearson_sums(x, y):
    """Sxx, Syy, Sxy of one pair's rows, centred and scaled as the device's pairwise kernel does it (DESIGN.md section
    9): each side's deviations from its mean, times the power of two (exact) that brings the largest into [0.5, 1),
    then Σd² - (Σd)²/m and Σde - Σd Σe/m, which take out what the rounding of the means leaves."""
    m = len(x)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return math.nan, math.nan, math.nan
    dev = []
    for v in (x, y):
        d = v - math.fsum(v) / m
        s = float(np.abs(d).max())
        dev.append(np.ldexp(d, -math.frexp(s)[1]) if s > 0 else d)
    d, e = dev
    sd, se = float(d.sum()), float(e.sum())
    return (float((d * d).sum()) - sd * sd / m, float((e * e).sum()) - se * se / m,
            float((d * e).sum()) - sd * se / m)


def _cor_pairs_numpy(X, pi, pj, method, pairwise, alternative, continuity):
    """The front end's path for engines without cor_pairs (the CPU tests' checker engines), pair by pair in numpy.
    Spearman: the device's exact integer sums of doubled ranks.  Pearson: the device's corrected and scaled sums
    (_pearson_sums), though not its summation order, so estimates agree with the device to rounding, not bit for bit.
    Returns (out3, reasons) like the HIP engine."""
    P = len(pi)
    out = np.full((P, 3), np.nan)
    rsn = np.zeros(P, dtype=np.int32)
    for p in range(P):
        x, y = X[:, pi[p]], X[:, pj[p]]
        joint = ~np.isnan(x) & ~np.isnan(y)
        x, y = x[joint], y[joint]
        n = len(x)
        out[p, 2] = n
        if n < (3 if (pairwise or method == "pearson") else 2):
            rsn[p] = _lib.COR_SHORT
            continue
        ties = False
        if method == "spearman":
            (x, tx), (y, ty) = _rank2(x), _rank2(y)
            ties = tx or ty
            x, y = x - (n + 1), y - (n + 1)
            sxx, syy, sxy = float((x * x).sum()), float((y * y).sum()), float((x * y).sum())
        else:
            if x.min() == x.max() or y.min() == y.max():
                sxx = syy = sxy = 0.0
            else:
                sxx, syy, sxy = _pearson_sums(x, y)
        if not (sxx > 0 and syy > 0) or math.isnan(sxy / math.sqrt(sxx * syy)):
            rsn[p] = _lib.COR_NA
            continue
        rho = min(1.0, max(-1.0, sxy / math.sqrt(sxx * syy)))
        if method == "spearman" and ties and n < 1290:
            rsn[p] = _lib.COR_TIES
        out[p, 0] = rho
        out[p, 1] = cor_test_pvalue(rho, n, method, alternative, continuity, ties)
    return out, rsn


_COR_ALTERNATIVES = ("two.sided", "less", "greater")


def cor_fast(x, y=None, use="everything", method="pearson", alternative="two.sided", continuity=False,
             include_only=None, return_matrix=True, colnames=None, engine=None):
    """stats::cor.test estimates and p-values for every pair of columns (R/other_correlations.R:27-141).

    Same arguments, defaults, NA policies, return shapes and error texts as the reference: ``use`` as in ``kt_fast``
    ("everything"/"all.obs": any NA -> every entry NA; "complete.obs": rows with an NA dropped first;
    "pairwise.complete.obs": per pair, and a pair with fewer than 3 joint rows is NA), ``method`` "pearson" or
    "spearman", self comparisons part of the result, ``include_only`` through ``setup_comparisons``.  Returns
    ``{"rho", "pvalue", "run_time"}`` (S x S, 0 outside the listed pairs) or, with ``return_matrix=False``,
    ``{"rho": data.frame(s1, s2, core, rho, pvalue, n_values), "run_time"}``.  Every pair runs on the MI355X
    (icikt_cor_pairs_f64); an ``engine`` without ``cor_pairs`` (CPU tests) gets the same arithmetic in numpy.
    Unlike the reference, ``n_values`` is each pair's own count (R/other_correlations.R:167 overwrites the whole
    vector with one pair's count).
    """
    if _lib.is_sparse(x):   # zero is a value here, not a missing cell: the dense matrix is what is meant
        x = _densify(x)
    na_method = _match_use(use)
    if na_method == "na.or.complete":
        raise ValueError("'na.or.complete' is not a supported value for `use`. "
                         "Please use one of all.obs complete.obs pairwise.complete everthing.")  # R/utils.R:86-90 (sic)
    if method not in ("pearson", "spearman"):
        raise ValueError("'arg' should be one of 'pearson', 'spearman'")
    if alternative not in _COR_ALTERNATIVES:
        raise ValueError("'arg' should be one of " + ", ".join(f"'{a}'" for a in _COR_ALTERNATIVES))
    if y is None:
        if not (pd is not None and isinstance(x, pd.DataFrame)) and np.ndim(x) < 2:
            raise ValueError("`x` and `y` should both be provided as vectors, or `x` should be matrix-like.")
        X, names = _as_matrix(x, colnames, "x", keep_dtype=True)
    else:
        if np.ndim(x) > 1 or np.ndim(y) > 1:
            raise ValueError("Both `x` and `y` must be vectors.")
        X = np.column_stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
        names = list(colnames) if colnames is not None else ["x", "y"]
    pi, pj, core = setup_comparisons(names, include_only, diag_good=False, ncore=1)
    P = len(pi)
    out = np.full((P, 3), np.nan)
    na_vals = np.isnan(X)
    do_computation = True
    if na_method in ("everything", "all.obs") and na_vals.any():
        do_computation = False
    if na_method == "complete.obs":
        keep = ~na_vals.any(axis=1)
        if keep.sum() == 0:
            do_computation = False
        else:
            X = np.asarray(X, dtype=np.float64)[keep]
    pairwise = na_method == "pairwise.complete.obs" and bool(np.isnan(X).any())
    t_diff = 0.0
    if do_computation:
        if not pairwise and X.shape[0] < (3 if method == "pearson" else 2):
            raise ValueError("not enough finite observations")  # stats::cor.test.default
        eng = engine or _default_engine()
        t1 = time.perf_counter()
        if hasattr(eng, "cor_pairs"):
            out, rsn = eng.cor_pairs(_for_engine(X, eng), pi, pj, method, pairwise, alternative, continuity)
        else:
            out, rsn = _cor_pairs_numpy(np.asarray(X, dtype=np.float64), pi, pj, method, pairwise, alternative, continuity)
        t_diff = time.perf_counter() - t1
        if (rsn == _lib.COR_TIES).any():
            warnings.warn(_COR_TIES_WARNING, RuntimeWarning, stacklevel=2)
    rho, pvalue, n_values = out[:, 0], out[:, 1], out[:, 2]
    if return_matrix:
        S = len(names)
        rm, pm = np.zeros((S, S)), np.zeros((S, S))
        rm[pi, pj] = rho
        rm[pj, pi] = rho
        pm[pi, pj] = pvalue
        pm[pj, pi] = pvalue
        return {"rho": _named_matrix(rm, names), "pvalue": _named_matrix(pm, names), "run_time": t_diff}
    names_arr = np.asarray(names, dtype=object)
    cols = {"s1": names_arr[pi], "s2": names_arr[pj], "core": core.astype(np.float64), "rho": rho, "pvalue": pvalue,
            "n_values": n_values}
    return {"rho": pd.DataFrame(cols) if pd is not None else cols, "run_time": t_diff}


# --------------------------------------------------------------------------------------------------
# missing-value diagnostics (R/left_censorship.R, R/rank-ordering.R) -- DESIGN.md section 10
# --------------------------------------------------------------------------------------------------
_R_NA_BITS = 0x7FF00000000007A2     # R's NA_real_
_R_NAN_BITS = 0x7FF8000000000000    # R_NaN
_LN_SQRT_2PI = 0.918938533204672741780329736406


def _bits(b):
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def _stirlerr(n):
    """log(n!) - log(sqrt(2 pi n) (n / e)^n), n >= 0 (Loader's stirlerr)."""
    if n == 0:
        return 0.0
    if n <= 15:
        return math.lgamma(n + 1.0) - (n + 0.5) * math.log(n) + n - _LN_SQRT_2PI
    nn = 1.0 / (n * n)
    return (1 / 12 - (1 / 360 - (1 / 1260 - (1 / 1680 - nn / 1188) * nn) * nn) * nn) / n


def _bd0(x, np_):
    """x log(x / np) + np - x without cancellation (Loader)."""
    if abs(x - np_) < 0.1 * (x + np_):
        v = (x - np_) / (x + np_)
        s = (x - np_) * v
        ej = 2 * x * v
        for j in range(1, 1000):
            ej *= v * v
            s1 = s + ej / (2 * j + 1)
            if s1 == s:
                return s1
            s = s1
        return s
    return x * math.log(x / np_) + np_ - x


def _dbinom(k, n, p):
    """P(X = k), X ~ Bin(n, p), to a relative accuracy that does not degrade with n (Loader's dbinom_raw)."""
    q = 1.0 - p
    if k == 0:
        return math.exp(n * math.log1p(-p)) if p < 0.5 else math.exp(n * math.log(q))
    if k == n:
        return math.exp(n * math.log(p))
    lc = _stirlerr(n) - _stirlerr(k) - _stirlerr(n - k) - _bd0(k, n * p) - _bd0(n - k, n * q)
    return math.exp(lc) * math.sqrt(n / (2 * math.pi * k * (n - k)))


def pbinom_upper(x, n, p=0.5):
    """P(X >= x), X ~ Bin(n, p): R's pbinom(x - 1, n, p, lower.tail = FALSE), through the incomplete beta
    I_p(x, n - x + 1) with its front factor from _dbinom."""
    x, n = int(x), int(n)
    if x <= 0:
        return 1.0
    if x > n:
        return 0.0
    a, b, q = float(x), float(n - x + 1), 1.0 - p
    if p > (a + 1) / (a + b + 2):
        return 1.0 - _incbeta_cf(b, a, q, p, front=_dbinom(x - 1, n, p) * p)   # 1 - P(X <= x - 1)
    return _incbeta_cf(a, b, p, q, front=_dbinom(x, n, p) * q)


def qbeta_binom_lower(alpha, x, n):
    """qbeta(alpha, x, n - x + 1) for 1 <= x <= n: the q with P(Bin(n, q) >= x) = alpha, by safeguarded Newton steps
    (the derivative of the tail in q is n dbinom(x - 1, n - 1, q))."""
    lo, hi = 0.0, 1.0
    q = min(max(x / n - 1.6448536269514722 * math.sqrt(max(x * (n - x), 1) / n ** 3), 1e-300), 1.0 - 1e-16)
    for _ in range(200):
        g = pbinom_upper(x, n, q) - alpha
        if g > 0:
            hi = q
        else:
            lo = q
        d = n * _dbinom(x - 1, n - 1, q) if n > 1 else 1.0
        step = g / d if d > 0 else math.inf
        qn = q - step
        if not (lo < qn < hi):
            qn = 0.5 * (lo + hi)
        if abs(qn - q) <= 2e-16 * q or hi - lo <= 2e-16 * hi:
            return qn
        q = qn
    return q


def _binom_test_greater(x, n):
    """stats::binom.test(x, n, p = 0.5, alternative = "greater")."""
    if n < 1 or x > n:
        raise ValueError("'n' must be a positive integer >= 'x'")
    return {
        "statistic": int(x), "statistic_name": "number of successes",
        "parameter": int(n), "parameter_name": "number of trials",
        "p_value": pbinom_upper(x, n, 0.5),
        "conf_int": (0.0 if x == 0 else qbeta_binom_lower(0.05, x, n), 1.0), "conf_level": 0.95,
        "estimate": x / n, "estimate_name": "probability of success",
        "null_value": 0.5, "alternative": "greater", "method": "Exact binomial test",
        "data_name": "total_success and total_trials",
    }


def _diag_matrix(data_matrix, colnames, arg):
    """_as_matrix for the diagnostics, which need no column names: (X, names, row labels or None)."""
    rows = None
    if pd is not None and isinstance(data_matrix, pd.DataFrame):
        rows = data_matrix.index
    elif colnames is None and _lib.is_sparse(data_matrix):
        colnames = list(range(data_matrix.shape[1]))
    elif colnames is None:
        colnames = list(range(np.shape(data_matrix)[1])) if np.ndim(data_matrix) == 2 else []
    X, names = _as_matrix(data_matrix, colnames, arg, keep_dtype=True, keep_sparse=True)
    return X, names, rows


def _class_levels(sample_classes, S, default):
    """split(., sample_classes) in factor() order: (levels, class index of every column).  Numbers sort numerically,
    strings as sorted() does (R's locale collation can order mixed-case labels differently)."""
    if sample_classes is None:
        labels = [default] * S
    else:
        labels = list(np.asarray(sample_classes, dtype=object).ravel())
        if len(labels) != S:
            raise ValueError("`sample_classes` must give one class per column")
    numeric = all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
                  for v in labels)
    if not numeric:
        labels = [str(v) for v in labels]
    levels = sorted(set(labels))
    pos = {v: i for i, v in enumerate(levels)}
    return levels, np.array([pos[v] for v in labels], dtype=np.int32)


def _device_rule(X, global_na):
    """The global_na rule as the device takes it: (X, global_na, host exclusion mask or None).  More than 32 distinct
    finite values: the host masks X (NaN) and passes NA alone."""
    vals = [] if global_na is None else [float(v) for v in np.atleast_1d(np.asarray(global_na, dtype=np.float64))]
    if not _host_masks(vals):
        return X, vals, None
    if _lib.is_sparse(X):
        X = _densify(X)
    X = np.asarray(X, dtype=np.float64)
    excl = setup_missing_matrix(X, vals)
    return _masked_fortran(X, excl), [math.nan], excl


def _r_median_sorted(v):
    """R's median of sorted values (no NA): NA when empty, a zero as +0, mean() of the middle two."""
    m = v.shape[0]
    if m == 0:
        return _bits(_R_NA_BITS)
    if m & 1:
        return float(v[m // 2]) + 0.0
    a, b = float(v[m // 2 - 1]), float(v[m // 2])
    s = a + b
    if math.isfinite(s):
        return 0.5 * s + 0.0
    if math.isfinite(a) and math.isfinite(b):
        return 0.5 * a + 0.5 * b
    return _bits(_R_NAN_BITS) if math.isnan(s) else s


def _col_medians_numpy(X, na_rm, miss=None):
    miss = np.isnan(X) if miss is None else miss
    out = np.empty(X.shape[1])
    for j in range(X.shape[1]):
        if miss[:, j].any() and not na_rm:
            out[j] = _bits(_R_NA_BITS)
        else:
            out[j] = _r_median_sorted(np.sort(X[~miss[:, j], j]))
    return out


def _censor_numpy(X, global_na, cls, n_class):
    excl = setup_missing_matrix(X, global_na)
    miss = excl | np.isnan(X)
    med = _col_medians_numpy(X, True, miss)
    trials = np.zeros(n_class, dtype=np.int64)
    success = np.zeros(n_class, dtype=np.int64)
    for k in range(n_class):
        cols = np.flatnonzero(cls == k)
        rows = miss[:, cols].any(axis=1)
        sub, mm, mk = X[rows][:, cols], miss[rows][:, cols], med[cols]
        valid = ~mm & ~np.isnan(mk)[None, :]
        with np.errstate(invalid="ignore"):
            trials[k] = int(valid.sum())
            success[k] = int((valid & (sub < mk[None, :])).sum())
    return trials, success, int(excl.sum())


def _rank2_na_first(col, miss):
    """2 * rank(col, na.last = FALSE) with the missing cells `miss` (integers)."""
    out = np.zeros(col.shape[0], dtype=np.int64)
    k = int(miss.sum())
    out[miss] = 2 * np.arange(1, k + 1)
    v = col[~miss] + 0.0   # -0 ties with 0
    if v.size:
        _u, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
        start = np.concatenate(([0], np.cumsum(cnt)[:-1]))
        out[~miss] = 2 * k + 2 * start[inv] + cnt[inv] + 1
    return out


def _rank_order_numpy(X, global_na, cols):
    Xc = X[:, cols]
    miss = setup_missing_matrix(Xc, global_na) | np.isnan(Xc)
    n, m = Xc.shape
    n_na = miss.sum(axis=1).astype(np.int32)
    kept = n_na < m
    rows = np.flatnonzero(kept)
    sub, msub = Xc[rows], miss[rows]
    med = np.full(n, _bits(_R_NA_BITS))
    if rows.size:
        r2 = np.column_stack([_rank2_na_first(sub[:, j], msub[:, j]) for j in range(m)])
        med[rows] = np.median(r2 / 2.0, axis=1)
    row_order = rows[np.argsort(-med[rows], kind="stable")].astype(np.int32)
    col_order = np.argsort(-msub.sum(axis=0), kind="stable").astype(np.int32)
    orig = np.array(sub, dtype=np.float64, order="F")
    orig[msub] = _bits(_R_NA_BITS)
    return {"n_kept": int(rows.size), "n_na": n_na, "median_rank": med, "row_order": row_order,
            "col_order": col_order, "original": orig,
            "ordered": np.asfortranarray(orig[np.searchsorted(rows, row_order)][:, col_order])}


def calculate_matrix_medians(in_matrix, use="col", na_rm=False, engine=None):
    """stats::median of every column (use = "row": of every row) of a numeric matrix (R/left_censorship.R:141-149).

    ``na_rm`` is median's na.rm: without it a column holding NaN gives NA.  An empty column gives NA; the mean of
    -Inf and Inf gives NaN.  Any ``use`` other than "row" means columns, as ``%in% "row"`` does.  Runs on the MI355X
    (icikt_col_medians_f64); an ``engine`` without ``col_medians`` gets the same arithmetic in numpy.  A sparse
    ``in_matrix`` goes to the device as its CSC arrays (absent cells are zeros, and zeros are values here);
    ``use="row"`` and any engine but the HIP one densify it with ``toarray()``.
    """
    X, _names, _rows = _diag_matrix(in_matrix, None, "in_matrix")
    if use == "row":
        X = (_densify(X) if _lib.is_sparse(X) else X).T
    eng = engine or _default_engine()
    if hasattr(eng, "col_medians"):
        return eng.col_medians(_for_engine(X, eng), na_rm)
    return _col_medians_numpy(np.asfortranarray(_densify(X) if _lib.is_sparse(X) else X, dtype=np.float64), na_rm)


def test_left_censorship(data_matrix, global_na=(float("nan"), float("inf"), 0), sample_classes=None, engine=None):
    """Binomial test of left censorship (R/left_censorship.R:35-128).

    A cell is missing when it is NaN or ``global_na`` excludes it (setup_missing_matrix).  Per class of
    ``sample_classes`` (default: one class "A"; classes in factor() order -- numbers numerically, strings as sorted()
    orders them, which R's locale collation can differ from for mixed-case labels), over the rows with a missing cell:
    ``trials`` counts the non-missing cells compared with their column's median (NA removed, over all rows of the
    column), ``success`` those below it.  Returns ``{"values": data.frame(trials, success, class), "binomial_test":
    binom.test(sum(success), sum(trials), p = 0.5, alternative = "greater")}``, or None (with a message) when the
    ``global_na`` rule excludes nothing.  The counts run on the MI355X (icikt_censor_counts_f64); an ``engine`` without
    ``censor_counts`` gets the same arithmetic in numpy.  A sparse ``data_matrix`` goes to the device as its CSC arrays;
    more than 32 finite ``global_na`` values and any engine but the HIP one densify it with ``toarray()``.
    """
    X, _names, _rows = _diag_matrix(data_matrix, None, "data_matrix")
    levels, cls = _class_levels(sample_classes, X.shape[1], "A")
    eng = engine or _default_engine()
    Xd, gna, excl = _device_rule(_for_engine(X, eng), global_na)
    if hasattr(eng, "censor_counts"):
        trials, success, n_ex = eng.censor_counts(Xd, gna, cls, len(levels))
    else:
        trials, success, n_ex = _censor_numpy(Xd, gna, cls, len(levels))
    if excl is not None:
        n_ex = int(excl.sum())
    if n_ex == 0:
        print("i `data_matrix` has no missing values, returning NULL")
        return None
    cols = {"trials": np.asarray(trials, dtype=np.int64), "success": np.asarray(success, dtype=np.int64),
            "class": np.array([str(v) for v in levels], dtype=object)}
    values = pd.DataFrame(cols) if pd is not None else cols
    return {"values": values, "binomial_test": _binom_test_greater(int(np.sum(success)), int(np.sum(trials)))}


test_left_censorship.__test__ = False   # a library function, not a pytest test


def rank_order_data(data_matrix, global_na=(float("nan"), float("inf"), 0), sample_classes=None, colnames=None,
                    engine=None):
    """Rank-ordered view of the missing values (R/rank-ordering.R:15-73).

    Per class of ``sample_classes`` (default: one class "rmf_abcd"): missing cells (NaN or excluded by ``global_na``)
    become NA, rows missing in every column of the class are dropped, each column is ranked with
    rank(x, na.last = FALSE), and the rows are ordered by their median rank (decreasing) and the columns by their
    share of NA (decreasing); both orders are stable.  A class returns ``{"original", "ordered", "n_na_rank":
    data.frame(n_na, median_rank[, split]), "row_order", "col_order"}`` -- the last two 0-based, an addition over the
    reference -- or None when no row is left.  One class returns its element, several a dict in class order.  Columns
    are split by position (the reference splits colnames(), which fails without column names).  Runs on the MI355X
    (icikt_rank_order_f64, one call per class); an ``engine`` without ``rank_order`` gets the same arithmetic in numpy.
    A sparse ``data_matrix`` goes to the device as its CSC arrays (column names from ``colnames=``); more than 32 finite
    ``global_na`` values and any engine but the HIP one densify it with ``toarray()``.
    """
    X, names, rows = _diag_matrix(data_matrix, colnames, "data_matrix")
    levels, cls = _class_levels(sample_classes, X.shape[1], "rmf_abcd")
    eng = engine or _default_engine()
    Xd, gna, _excl = _device_rule(_for_engine(X, eng), global_na)
    row_labels = np.asarray(rows) if rows is not None else np.arange(X.shape[0])
    out = {}
    for k, level in enumerate(levels):
        cols = np.flatnonzero(cls == k).astype(np.int32)
        if hasattr(eng, "rank_order"):
            r = eng.rank_order(Xd, gna, cols)
        else:
            r = _rank_order_numpy(Xd, gna, cols)
        if r["n_kept"] == 0:
            out[level] = None
            continue
        kept = np.flatnonzero(r["n_na"] < len(cols))
        cnames = [names[j] for j in cols]
        n_na_rank = {"n_na": r["n_na"][kept], "median_rank": r["median_rank"][kept]}
        if level != "rmf_abcd":
            n_na_rank["split"] = np.array([str(level)] * kept.size, dtype=object)
        if pd is not None:
            original = pd.DataFrame(r["original"], index=row_labels[kept], columns=cnames)
            ordered = pd.DataFrame(r["ordered"], index=row_labels[r["row_order"]],
                                   columns=[cnames[j] for j in r["col_order"]])
            n_na_rank = pd.DataFrame(n_na_rank, index=row_labels[kept])
        else:
            original, ordered = r["original"], r["ordered"]
        out[level] = {"original": original, "ordered": ordered, "n_na_rank": n_na_rank,
                      "row_order": np.asarray(r["row_order"]), "col_order": np.asarray(r["col_order"])}
    if len(out) == 1:
        return next(iter(out.values()))
    return out
