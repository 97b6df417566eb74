"""Timing of the missing-value diagnostics' device entries (icikt_col_medians_f64, icikt_censor_counts_f64,
icikt_rank_order_f64) against the numpy restatement of the package (development aid).

    python tools/diag_time.py [--reps 3] [--json out.json]

Shapes 10 000 x 1 024 and 50 000 x 2 048 with 10 % and 30 % missing cells (NaN and zeros, more of them in the low rows:
left-censored), two classes.  Per entry: the median wall time of the host call, the per-kernel ms of the same calls
from ICIKT_FLAG_TIMING (prepare = the matrix's H2D, passes = column and row passes, gather = original / ordered), the
H2D share of the wall time, and the numpy path's time for the same work (once)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from icikendalltau_amd import _lib, api  # noqa: E402

GNA = (float("nan"), float("inf"), 0.0)


def make(n, S, frac, seed):
    rng = np.random.default_rng(seed)
    X = np.sort(rng.lognormal(10, 1, size=n))[:, None] + rng.normal(0, 0.1, size=(n, S))
    p = frac * 2 * (1 - np.arange(n) / n)[:, None]   # more missing at the low end
    u = rng.random((n, S))
    X[u < p / 2] = np.nan
    X[(u >= p / 2) & (u < p)] = 0.0
    return np.asfortranarray(X)


def timed(ctx, fn, reps):
    walls, ks = [], []
    for _ in range(reps):
        ctx.reset_timers()
        t0 = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t0) * 1e3)
        ks.append([ctx.kernel_ms(k)[0] for k in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    i = int(np.argsort(walls)[len(walls) // 2])
    wall, (h2d, passes, gather) = walls[i], ks[i]
    return {"wall_ms": round(wall, 3), "h2d_ms": round(h2d, 3), "passes_ms": round(passes, 3),
            "gather_ms": round(gather, 3), "h2d_share": round(h2d / wall, 3) if wall else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = _lib.default_context()
    rows = []
    for n, S in ((10_000, 1_024), (50_000, 2_048)):
        for frac in (0.1, 0.3):
            X = make(n, S, frac, n + S)
            cls = (np.arange(S) >= S // 2).astype(np.int32)
            halves = [np.flatnonzero(cls == k).astype(np.int32) for k in (0, 1)]
            F = _lib.FLAG_TIMING
            ctx.col_medians(X[:, :8], True)   # warm-up
            cases = {
                "col_medians": lambda: ctx.col_medians(X, True, flags=F),
                "censor_counts": lambda: ctx.censor_counts(X, GNA, cls, 2, flags=F),
                "rank_order (per class)": lambda: [ctx.rank_order(X, GNA, c, flags=F) for c in halves],
            }
            cpu = {
                "col_medians": lambda: api._col_medians_numpy(X, True),
                "censor_counts": lambda: api._censor_numpy(X, GNA, cls, 2),
                "rank_order (per class)": lambda: [api._rank_order_numpy(X, GNA, c) for c in halves],
            }
            for name, fn in cases.items():
                r = timed(ctx, fn, a.reps)
                t0 = time.perf_counter()
                cpu[name]()
                r["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                r.update({"entry": name, "shape": f"{n}x{S}", "missing": frac, "bytes": X.nbytes})
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
