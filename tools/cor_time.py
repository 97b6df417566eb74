"""Timing of cor_fast's device entry (icikt_cor_pairs_f64) on the c4 shape, with a numpy / scipy CPU baseline on a
subset of the pairs (development aid).

    python tools/cor_time.py [--reps 5] [--json out.json]

Cases: Pearson and Spearman x use = "everything" (no NA, all pairs + self pairs: the tile kernel) and
"pairwise.complete.obs" with ~10 % NA, and include_only with one column against all.  Per case: the median wall time of
the host entry (H2D of the matrix, the three kernels, D2H), pairs/s, and the per-kernel ms of the same calls."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from scipy import stats  # noqa: E402

from icikendalltau_amd import _lib, api  # noqa: E402


def make(n, S, na, seed):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    if na:
        X[rng.random(X.shape) < na] = np.nan
    return X


def cpu_baseline(X, pi, pj, method, k=2000):
    """scipy pearsonr / spearmanr + p-value on k pairs of the list, per pair, as cor_split loops over cor.test."""
    sel = np.linspace(0, len(pi) - 1, min(k, len(pi))).astype(int)
    f = stats.pearsonr if method == "pearson" else stats.spearmanr
    t0 = time.perf_counter()
    for p in sel:
        x, y = X[:, pi[p]], X[:, pj[p]]
        ok = ~np.isnan(x) & ~np.isnan(y)
        f(x[ok], y[ok])
    return len(sel) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    names = [f"s{i}" for i in range(a.S)]
    full = api.setup_comparisons(names, None, diag_good=False)[:2]
    one = api.setup_comparisons(names, ["s0"], diag_good=False)[:2]
    rows = []
    for method in ("pearson", "spearman"):
        for use, na, (pi, pj) in (("everything", 0.0, full), ("pairwise.complete.obs", 0.1, full),
                                  ("include_only 1 vs all", 0.0, one)):
            X = make(a.n, a.S, na, 4)
            ctx.cor_pairs(X, pi, pj, method, na > 0)   # warm-up: buffers, code objects
            walls, ks = [], []
            for _ in range(a.reps):
                ctx.reset_timers()
                t0 = time.perf_counter()
                ctx.cor_pairs(X, pi, pj, method, na > 0, flags=_lib.FLAG_TIMING)
                walls.append(time.perf_counter() - t0)
                ks.append([ctx.kernel_ms(i)[0] for i in range(3)])
            w = float(np.median(walls))
            k = np.median(np.array(ks), axis=0)
            row = {"method": method, "use": use, "n": a.n, "S": a.S, "pairs": len(pi), "wall_ms": w * 1e3,
                   "pairs_per_s": len(pi) / w, "prepare_ms": k[0], "products_ms": k[1], "epilogue_ms": k[2],
                   "cpu_pairs_per_s": cpu_baseline(X, pi, pj, method)}
            rows.append(row)
            print(f"{method:8s} {use:24s} P={len(pi):7d} wall={w * 1e3:8.2f} ms  {len(pi) / w:.3e} pairs/s  "
                  f"prepare={k[0]:.2f} products={k[1]:.2f} epilogue={k[2]:.2f} ms  "
                  f"cpu(scipy)={row['cpu_pairs_per_s']:.3e} pairs/s", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
