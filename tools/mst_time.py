"""What the spanning-tree entry costs, on one MI355X, both routes in one process on the same card:

  1. the bar: Context.mst against the route a caller had before it -- Context.matrix over all pairs, then
     scipy.sparse.csgraph.minimum_spanning_tree over the triangle of 2 - raw on the host -- at S = 4 096, n = 2 000,
     F-ordered float64; the legs alternate; the same with the triangle cut into 8 blocks (tkblock);
  2. with ICIKT_FLAG_TIMING, per shape: the pair kernel's time (ICIKT_K_PAIRS), the time under ICIKT_K_EPILOGUE (pair
     epilogue + statistics + keep + rounds + the tree's pair run), the same for a call with min_raw = +Inf -- the keep
     and ONE round that finds nothing, no tree run -- and their difference: the rounds beyond the first and the tree's
     pair run.  n_rounds is recorded;
  3. S = 32 768, n = 256 (5.4e8 pairs, a kept plane of 4.3 GB): the new route only, median of 3.

    python tools/mst_time.py [--repeats 20] [--out profiles/mst_time.log]
    python tools/mst_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
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
from medians_time import make   # noqa: E402


def old_route(ctx, X):
    """The full matrices, then scipy's minimum spanning tree of the upper triangle of 2 - raw (positive for every pair:
    a zero would be no edge to scipy); returns the tree's raw values, sorted"""
    from scipy.sparse.csgraph import minimum_spanning_tree
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    W = np.triu(2.0 - out5[1], k=1)
    W[np.isnan(W)] = 0.0
    T = minimum_spanning_tree(W).tocoo()
    return np.sort(out5[1][T.row, T.col])


def time_bar(ctx, log, X, repeats, spec=None, warm=2):
    ctx.debug_set_plan(spec)
    ta, tb = [], []
    for i in range(warm + repeats):
        t0 = time.perf_counter()
        old = old_route(ctx, X)
        t1 = time.perf_counter()
        new = ctx.mst(X)
        t2 = time.perf_counter()
        if i >= warm:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
    ctx.debug_set_plan(None)
    sa, sb = stats(ta), stats(tb)
    same = bool(np.array_equal(old, np.sort(new[2][1])))   # every maximum spanning tree has the same multiset of weights
    log(f"  (a) Context.matrix + scipy minimum_spanning_tree: {fmt(sa)}")
    log(f"  (b) Context.mst:                                  {fmt(sb)}   tree weights {'equal' if same else 'DIFFER'}, "
        f"n_rounds {new[5]}")
    log(f"  new route {sa[0] / sb[0]:.2f}x the old one's speed at the median: {'NOT SLOWER' if sb[0] <= sa[0] else 'SLOWER'}")
    return sb[0] <= sa[0]


def time_shares(ctx, log, X, repeats, spec=None, warm=2):
    """wall time and, per call, ms under ICIKT_K_PAIRS and ICIKT_K_EPILOGUE, for the whole call and for min_raw = +Inf"""
    ctx.debug_set_plan(spec)
    res = {}
    for name, min_raw in (("whole tree", None), ("min_raw=+Inf", float("inf"))):
        ts, shares, rounds = [], [], 0
        for i in range(warm + repeats):
            ctx.reset_timers()
            t0 = time.perf_counter()
            out = ctx.mst(X, min_raw, flags=_lib.FLAG_TIMING)
            t1 = time.perf_counter()
            rounds = out[5]
            if i >= warm:
                ts.append(t1 - t0)
                shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
        med = np.median(np.asarray(shares), axis=0)
        res[name] = med
        log(f"  {str(spec or 'default'):12s} {name:12s} {fmt(stats(ts))}; per call: copies + pre-pass {med[0]:8.2f} ms, pair "
            f"kernel {med[1]:8.2f} ms, epilogue + statistics + keep + rounds + tree run {med[2]:8.2f} ms; n_rounds {rounds}")
    ctx.debug_set_plan(None)
    log(f"  {str(spec or 'default'):12s} the rounds beyond the first and the tree's pair run: "
        f"{res['whole tree'][2] - res['min_raw=+Inf'][2]:+.2f} ms per call")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S = (2000, 4096) if not a.quick else (100, 256)
    big_n, big_S = (256, 32768) if not a.quick else (32, 1024)
    ctx = _lib.Context(0)
    log(f"# tools/mst_time.py: median of {a.repeats} calls per leg after 2 warm-up calls, one process, one card; host "
        f"clock around calls that end in a stream synchronisation; seeded generators"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    P = S * (S - 1) // 2
    cut = f"tkblock={P // 8 + 1}"
    oks = []
    for name, spec in (("one block", None), ("8 blocks", cut)):
        log(f"\n## 1. the bar: S = {S}, n = {n} ({P} pairs), F-ordered float64, {name}")
        oks.append(time_bar(ctx, log, X, a.repeats, spec))
    log("\n## 2. time shares of the new entry (ICIKT_FLAG_TIMING)")
    log(f"  S = {S}, n = {n}")
    for spec in (None, cut):
        time_shares(ctx, log, X, a.repeats, spec)
    log(f"\n## 3. S = {big_S}, n = {big_n} ({big_S * (big_S - 1) // 2} pairs), the new route only, median of 3")
    Xb = make(big_n, big_S, 7)
    time_shares(ctx, log, Xb, 3, None, warm=1)
    log("\n# the new entry not slower than the old route: "
        + ", ".join(f"{name} " + ("YES" if ok else "NO") for name, ok in zip(("one block", "8 blocks"), oks)))
    ctx.close()


if __name__ == "__main__":
    main()
