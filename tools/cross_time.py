"""What the cross entry costs, on one MI355X, all routes in one process on the same card: a
query of Sq = 64 samples against a reference of Sr = 4 096, n = 2 000, k = 32, F-ordered float64.

  (a) Context.topk on the stacked matrix: all C(Sq + Sr, 2) pairs, then the query rows of the result -- whose partners
      may be other QUERY samples, so it does not even answer the question;
  (b) Context.pairs on the stacked matrix with the rectangle's explicit pair list, then the selection in numpy;
  (c) Context.cross, top-k only, and with the five matrices as well.

The legs alternate.  With ICIKT_FLAG_TIMING, route (c)'s time per kernel class: copies + pre-pass, pair kernel, pair
epilogue + folds.

    python tools/cross_time.py [--repeats 20] [--out profiles/cross_time.log]
    python tools/cross_time.py --quick       # tiny shapes: a rehearsal of the script, not a measurement
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np   # noqa: E402

from icikendalltau_amd import _lib   # noqa: E402
from ingest_time import Tee, fmt, stats   # noqa: E402


def make(n, S, seed):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X


def route_topk(ctx, X, Sq, k):
    idx, vals, _nv, _mx, _rc = ctx.topk(X, k)
    return idx[:Sq], vals[:, :Sq]


def route_pairs(ctx, X, pi, pj, Sq, Sr, k):
    """the rectangle as a flat pair list, then per query the k largest raw (argpartition, then a sort of the k)"""
    out, _cnt, _rsn = ctx.pairs(X, pi, pj, want_counts=False)
    raw = out[:, 0].reshape(Sq, Sr).copy()
    raw[np.isnan(raw)] = -np.inf
    part = np.argpartition(-raw, k - 1, axis=1)[:, :k]
    rows = np.arange(Sq)[:, None]
    order = np.argsort(-raw[rows, part], axis=1, kind="stable")
    idx = part[rows, order]
    return idx, out.reshape(Sq, Sr, 4)[rows, idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, Sq, Sr, k = (200, 8, 256, 8) if a.quick else (2000, 64, 4096, 32)
    warm = 2
    ctx = _lib.Context(0)
    log(f"# tools/cross_time.py: median of {a.repeats} calls per leg after {warm} warm-up calls, one process, one card; host "
        f"clock around calls that end in a stream synchronisation; seeded generators"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    Q, R = make(n, Sq, 1), make(n, Sr, 2)
    X = np.asfortranarray(np.hstack([Q, R]))
    pi = np.repeat(np.arange(Sq, dtype=np.int32), Sr)
    pj = (Sq + np.tile(np.arange(Sr, dtype=np.int32), Sq)).astype(np.int32)
    log(f"\n## Sq = {Sq}, Sr = {Sr}, n = {n}, k = {k}, F-ordered float64: {Sq * Sr} pairs of the rectangle, "
        f"{(Sq + Sr) * (Sq + Sr - 1) // 2} of the stacked triangle")
    ta, tb, tc, td = [], [], [], []
    for i in range(warm + a.repeats):
        t0 = time.perf_counter()
        route_topk(ctx, X, Sq, k)
        t1 = time.perf_counter()
        rb = route_pairs(ctx, X, pi, pj, Sq, Sr, k)
        t2 = time.perf_counter()
        rc = ctx.cross(Q, R, k, want_matrix=False)
        t3 = time.perf_counter()
        ctx.cross(Q, R, k, want_matrix=True)
        t4 = time.perf_counter()
        if i >= warm:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
            tc.append(t3 - t2)
            td.append(t4 - t3)
    same = bool(np.array_equal(rb[1][:, :, 0], rc[2][1]))     # (the raw values picked; indices may differ among equal raw)
    sa, sb, sc, sd = stats(ta), stats(tb), stats(tc), stats(td)
    log(f"  (a) Context.topk on the stacked matrix:                       {fmt(sa)}")
    log(f"  (b) Context.pairs, explicit list + numpy selection:           {fmt(sb)}")
    log(f"  (c) Context.cross, top-k only:                                {fmt(sc)}   raw of the picks {'equal' if same else 'DIFFERS'} to (b)'s")
    log(f"      Context.cross, top-k and the five {Sq} x {Sr} matrices:    {fmt(sd)}")
    log(f"  (c) is {sa[0] / sc[0]:.2f}x route (a)'s speed and {sb[0] / sc[0]:.2f}x route (b)'s at the median")
    log("\n## route (c) per kernel class (ICIKT_FLAG_TIMING)")
    for want_matrix in (False, True):
        shares = []
        for i in range(warm + a.repeats):
            ctx.reset_timers()
            ctx.cross(Q, R, k, want_matrix=want_matrix, flags=_lib.FLAG_TIMING)
            if i >= warm:
                shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
        med = np.median(np.asarray(shares), axis=0)
        log(f"  {'top-k and matrices' if want_matrix else 'top-k only':20s} copies + pre-pass {med[0]:8.3f} ms, pair kernel {med[1]:8.3f} ms, "
            f"pair epilogue + folds {med[2]:8.3f} ms")
    es = []
    for i in range(warm + a.repeats):
        ctx.reset_timers()
        ctx.pairs(X, pi, pj, flags=_lib.FLAG_TIMING, want_counts=False)
        if i >= warm:
            es.append(ctx.kernel_ms(_lib.K_EPILOGUE)[0])
    log(f"  pair epilogue alone (Context.pairs, the same pair list): median {np.median(es):8.3f} ms per call")
    ctx.close()


if __name__ == "__main__":
    main()
