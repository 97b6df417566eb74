"""Case generator of the seeded diagnostics / cor_fast sweep (tests/test_gpu_diag_cor_sweep.py): a shape from the
lengths where the kernels change shape, a value model, missing cells, a global_na set, class labels and a cor_fast
mode; the three diagnostics and cor_pairs against tests/diag_checker.py and tests/cor_checker.py."""
import math
import os
import traceback

import numpy as np

from tests import diag_checker as dc
from tests import launch_caps as lc
from tests.cor_checker import assert_matches_exact, check_pairs

LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536,
           65537, 131073, 262144]
MODELS = ("lognormal", "ties", "inf_zero", "extreme", "missing")


def _values(rng, n, S, model):
    if model == "lognormal":           # left-censored: the low values missing
        X = rng.lognormal(2, 1, size=(n, S))
        X[X < rng.uniform(1, 5)] = np.nan
    elif model == "ties":
        X = rng.integers(0, 5, size=(n, S)).astype(np.float64)
    elif model == "inf_zero":
        X = rng.normal(size=(n, S))
        pick = rng.random((n, S))
        X[pick < 0.05] = np.inf
        X[(pick >= 0.05) & (pick < 0.1)] = -np.inf
        X[(pick >= 0.1) & (pick < 0.15)] = 0.0
        X[(pick >= 0.15) & (pick < 0.2)] = -0.0
    elif model == "extreme":
        X = rng.normal(size=(n, S)) * np.where(rng.random((1, S)) < 0.5, 1e300, 1e-300)
    else:
        X = rng.normal(size=(n, S))
        X[:, rng.random(S) < 0.3] = np.nan
        X[rng.random(n) < 0.3, :] = np.nan
    return X


def _global_na(rng):
    k = int(rng.integers(0, 5))
    vals = [math.nan, math.inf, 0.0, -0.0, 1.0, 2.0, 3.0, -math.inf][:8]
    gna = list(rng.choice(np.array(vals), size=k, replace=False)) if k else []
    if rng.random() < 0.1:
        gna = [math.nan] + [float(v) for v in range(31)]     # 32 values
    return tuple(float(v) for v in gna)


def draw(rng):
    n = int(rng.choice(LENGTHS))
    if n <= 64 and rng.random() < 0.25:
        S = int(rng.integers(2049, 2300))                       # short and wide: past the fixed caps
    else:
        S = int(rng.integers(1, max(2, min(40, 2_000_000 // n))))
    model = str(rng.choice(MODELS))
    X = _values(rng, n, S, model)
    X[rng.random((n, S)) < rng.choice([0.0, 0.05, 0.3])] = np.nan
    return np.asfortranarray(X), model


def one_case(ctx, rng, case, out_dir, cor=True):
    X, model = draw(rng)
    n, S = X.shape
    gna = _global_na(rng)
    n_class = int(rng.integers(1, min(S, 40) + 1))
    cls = rng.integers(0, n_class, size=S)
    extra = int(rng.integers(0, 3))                             # n_class above the largest label used
    label = f"case {case}: {n}x{S} {model} gna={gna} classes={n_class}+{extra}"
    try:
        for na_rm in (False, True):
            dc.assert_col_medians(ctx.col_medians(X, na_rm, global_na=gna), X, na_rm, gna, label)
        dc.assert_censor(ctx.censor_counts(X, gna, cls, n_class + extra, want_medians=True), X, gna, cls,
                         n_class + extra, label)
        k = int(rng.integers(0, n_class))
        cols = np.flatnonzero(cls == k).astype(np.int32)
        if cols.size and rng.random() < 0.3:
            cols = rng.permutation(cols).astype(np.int32)
        if cols.size:
            dc.assert_rank_order(ctx.rank_order(X, gna, cols), X, gna, cols, label)
        if cor:
            _cor_case(ctx, rng, X, model, label)
    except AssertionError as e:
        path = os.path.join(out_dir, f"diag_cor_case{case}.npz")
        np.savez(path, X=X, gna=np.array(gna), cls=cls)
        where = traceback.extract_tb(e.__traceback__)[-1]
        return f"{label}: {str(e).strip()[:400]} at {where.name}:{where.lineno} (input {path})"
    return None


def _cor_case(ctx, rng, X, model, label):
    n, S = X.shape
    if S < 2 or n < 2:
        return
    method = str(rng.choice(["pearson", "spearman"]))
    pairwise = bool(rng.random() < 0.5)
    if model == "extreme" and method == "pearson" and n * S > 20000:
        return                                                 # exact arithmetic only: keep it small
    if not pairwise:                                           # the dense route takes no NA (cor_fast's everything)
        X = X.copy()
        X[np.isnan(X)] = 1.0
        if method == "pearson":
            X[~np.isfinite(X)] = 2.0
        if n < 3:
            return
    if rng.random() < 0.5 and S <= 60:
        pi, pj = lc.combn(S)
    else:
        P = int(rng.integers(1, 200))
        pi = rng.integers(0, S, size=P).astype(np.int32)
        pj = rng.integers(0, S, size=P).astype(np.int32)
    budget = max(1, 3_000_000 // max(n, 1))                    # pairs the host reference checks
    sel = np.arange(len(pi)) if len(pi) <= budget else np.sort(rng.choice(len(pi), budget, replace=False))
    got, _ = ctx.cor_pairs(X, pi, pj, method, pairwise)
    exact = method == "pearson" and n * len(sel) <= 200_000
    want, _ = check_pairs(X, pi[sel], pj[sel], method, pairwise, exact=exact)
    if exact:
        assert_matches_exact(got[sel, 0], got[sel, 1], got[sel, 2], want, label=f"{label} cor pearson exact")
    else:
        lc.assert_pairs(got[sel], want, f"{label} cor {method} pairwise={pairwise}")
