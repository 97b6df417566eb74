"""What the complete / average linkage entry costs, on one MI355X, both routes in one process on
the same card:

  1. the bar: Context.hclust against the route a caller had before it -- Context.matrix over all pairs, then
     scipy.cluster.hierarchy.linkage(squareform(1 - raw), method) on the host -- for "complete" and "average" at
     S = 4 096, n = 2 000, F-ordered float64; the legs alternate; median of 20;
  2. with ICIKT_FLAG_TIMING, per method: the pair kernel's time (ICIKT_K_PAIRS) and the time under ICIKT_K_EPILOGUE for
     the whole call and for a call with min_raw = +Inf, whose first pick ends the call so that its other 3 (S - 1) - 1
     launches return at once; and Context.mst with min_raw = +Inf, which is the same pair epilogue, statistics and keep
     with one small kernel behind them.  The differences are the split the timers allow:
       hclust(+Inf) - mst(+Inf)      expand + first scan + the floor of 3 (S - 1) launches
       hclust(whole) - hclust(+Inf)  what the steps' work adds to that floor
  3. S = 32 768, n = 256 (5.4e8 pairs, a kept plane of 4.3 GB and a table of 8.6 GB): the new route only, median of 3.

    python tools/hclust_time.py [--repeats 20] [--out profiles/hclust_time.log]
    python tools/hclust_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
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

METHODS = ("complete", "average")


def old_route(ctx, X, method):
    """The full matrices, then scipy's linkage of the condensed 1 - raw; returns the linkage matrix"""
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    D = 1.0 - out5[1]
    np.fill_diagonal(D, 0.0)
    D[np.isnan(D)] = 2.0           # (a pair without a raw: as far apart as tau allows, where the entry refuses the merge)
    return linkage(squareform(D, checks=False), method)


def time_bar(ctx, log, X, method, repeats, warm=2):
    ta, tb = [], []
    for i in range(warm + repeats):
        t0 = time.perf_counter()
        Z = old_route(ctx, X, method)
        t1 = time.perf_counter()
        new = ctx.hclust(X, method)
        t2 = time.perf_counter()
        if i >= warm:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
    sa, sb = stats(ta), stats(tb)
    # where no two similarities tie both routes make the same tree; the heights agree to rounding (average) or exactly
    err = float(np.max(np.abs(np.sort(1.0 - new[3]) - np.sort(Z[:, 2])))) if len(new[3]) == Z.shape[0] else float("nan")
    log(f"  (a) Context.matrix + scipy linkage({method!r}): {fmt(sa)}")
    log(f"  (b) Context.hclust(method={method!r}):          {fmt(sb)}   n_merges {len(new[0])}, largest difference of "
        f"the sorted heights {err:.3g}")
    log(f"  new route {sa[0] / sb[0]:.2f}x the old one's speed at the median: {'NOT SLOWER' if sb[0] <= sa[0] else 'SLOWER'}")
    return sb[0] <= sa[0]


def _shares(ctx, call, repeats, warm):
    ts, shares = [], []
    for i in range(warm + repeats):
        ctx.reset_timers()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if i >= warm:
            ts.append(t1 - t0)
            shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    return stats(ts), np.median(np.asarray(shares), axis=0)


def time_shares(ctx, log, X, method, repeats, warm=2):
    S = X.shape[1]
    inf = float("inf")
    legs = (("hclust whole", lambda: ctx.hclust(X, method, flags=_lib.FLAG_TIMING)),
            ("hclust min_raw=+Inf", lambda: ctx.hclust(X, method, inf, flags=_lib.FLAG_TIMING)),
            ("mst min_raw=+Inf", lambda: ctx.mst(X, inf, flags=_lib.FLAG_TIMING)))
    med = {}
    for name, call in legs:
        st, med[name] = _shares(ctx, call, repeats, warm)
        log(f"  {method:9s} {name:20s} {fmt(st)}; per call: copies + pre-pass {med[name][0]:9.2f} ms, pair kernel "
            f"{med[name][1]:9.2f} ms, ICIKT_K_EPILOGUE {med[name][2]:9.2f} ms")
    floor = med["hclust min_raw=+Inf"][2] - med["mst min_raw=+Inf"][2]
    work = med["hclust whole"][2] - med["hclust min_raw=+Inf"][2]
    log(f"  {method:9s} split: pair kernel {med['hclust whole'][1]:.2f} ms; expand + first scan + the floor of "
        f"{3 * (S - 1)} launches {floor:+.2f} ms; what the steps' work adds {work:+.2f} ms")


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
    log(f"# tools/hclust_time.py: median of {a.repeats} calls per leg after 2 warm-up calls, one process, one card; host "
        f"clock around calls that end in a stream synchronisation; seeded generators"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    P = S * (S - 1) // 2
    oks = []
    for method in METHODS:
        log(f"\n## 1. the bar: S = {S}, n = {n} ({P} pairs), F-ordered float64, {method}")
        oks.append(time_bar(ctx, log, X, method, a.repeats))
    log(f"\n## 2. time shares of the new entry (ICIKT_FLAG_TIMING), S = {S}, n = {n}")
    for method in METHODS:
        time_shares(ctx, log, X, method, a.repeats)
    log(f"\n## 3. S = {big_S}, n = {big_n} ({big_S * (big_S - 1) // 2} pairs), the new route only, median of 3")
    Xb = make(big_n, big_S, 7)
    for method in METHODS:
        time_shares(ctx, log, Xb, method, 3, warm=1)
    log("\n# the new entry not slower than the old route at S = %d: " % S
        + ", ".join(f"{m} " + ("YES" if ok else "NO") for m, ok in zip(METHODS, oks)))
    ctx.close()


if __name__ == "__main__":
    main()
