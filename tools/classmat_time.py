"""What the class-matrix entry costs, on one MI355X, both routes in one process on the same card:

  1. the bar: Context.class_matrix against the route a caller had before it -- Context.matrix over all pairs, then
     np.nanmedian over each class's block of columns of cor and of raw on the host -- at S = 4 096, n = 2 000, F-ordered
     float64, for (a) one class, (b) 16 classes of 256 samples and (c) 2 048 classes of 2; the legs alternate;
  2. with ICIKT_FLAG_TIMING, the new entry's time under ICIKT_K_PREPARE (copies + pre-pass), ICIKT_K_PAIRS (the pair
     kernel) and ICIKT_K_EPILOGUE (pair epilogue + statistics + keep + select) at the three layouts, the pair epilogue
     alone, and 16 classes of 256 with every pass re-reading the kept plane (medlds=0).
  The layout (c) is the small-class question: 8.4 million workgroups of 256 threads for two keys each.

    python tools/classmat_time.py [--repeats 20] [--out profiles/classmat_time.log]
    python tools/classmat_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
"""
import argparse
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np   # noqa: E402

from icikendalltau_amd import _lib   # noqa: E402
from ingest_time import Tee, fmt, stats   # noqa: E402
from medians_time import epilogue_alone, make   # noqa: E402


def old_route(ctx, X, cls, n_class):
    """The full matrices, then per class np.nanmedian over the rows of its block of columns of cor and of raw (a
    member's own cell out)"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    S = X.shape[1]
    med2 = np.full((2, S, n_class), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # (an all-NaN slice: a singleton's own cell)
        for k in range(n_class):
            members = np.nonzero(cls == k)[0]
            if len(members) == 0:
                continue
            for q in (0, 1):
                block = out5[q][:, members]
                block[members, np.arange(len(members))] = np.nan
                med2[q, :, k] = np.nanmedian(block, axis=1)
    return med2


def time_bar(ctx, log, X, cls, n_class, repeats, warm=2):
    ta, tb = [], []
    for i in range(warm + repeats):
        t0 = time.perf_counter()
        old = old_route(ctx, X, cls, n_class)
        t1 = time.perf_counter()
        new = ctx.class_matrix(X, cls, n_class)
        t2 = time.perf_counter()
        if i >= warm:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
    sa, sb = stats(ta), stats(tb)
    same = bool(np.array_equal(old[1], new[0][1]))   # med_raw (nanmedian's midpoint of two is the same correctly rounded one)
    log(f"  (a) Context.matrix + np.nanmedian per class block: {fmt(sa)}")
    log(f"  (b) Context.class_matrix:                          {fmt(sb)}   med_raw {'equal' if same else 'DIFFERS'}")
    log(f"  new route {sa[0] / sb[0]:.2f}x the old one's speed at the median: {'NOT SLOWER' if sb[0] <= sa[0] else 'SLOWER'}")
    return sb[0] <= sa[0]


def time_shares(ctx, log, X, cls, n_class, repeats, spec=None, warm=2):
    """wall time and, per call, ms under ICIKT_K_PREPARE / _PAIRS / _EPILOGUE (keep and select are in the last)"""
    ctx.debug_set_plan(spec)
    ts, shares = [], []
    for i in range(warm + repeats):
        ctx.reset_timers()
        t0 = time.perf_counter()
        ctx.class_matrix(X, cls, n_class, flags=_lib.FLAG_TIMING)
        t1 = time.perf_counter()
        if i >= warm:
            ts.append(t1 - t0)
            shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    ctx.debug_set_plan(None)
    med = np.median(np.asarray(shares), axis=0)
    log(f"  {str(spec or 'default'):10s} {fmt(stats(ts))}; per call: copies + pre-pass {med[0]:8.2f} ms, pair kernel "
        f"{med[1]:8.2f} ms, pair epilogue + statistics + keep + select {med[2]:8.2f} ms")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S, per = (2000, 4096, 256) if not a.quick else (100, 256, 16)
    ctx = _lib.Context(0)
    log(f"# tools/classmat_time.py: median of {a.repeats} calls per leg after 2 warm-up calls, one process, one card; host "
        f"clock around calls that end in a stream synchronisation; seeded generators"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    layouts = (("one class", np.zeros(S, dtype=np.int32), 1),
               (f"{S // per} classes of {per}", (np.arange(S) // per).astype(np.int32), S // per),
               (f"{S // 2} classes of 2", (np.arange(S) // 2).astype(np.int32), S // 2))
    oks = []
    for name, cls, n_class in layouts:
        log(f"\n## 1. the bar: S = {S}, n = {n}, {name} ({S * n_class} cells, {S * (S - 1) // 2} pairs), F-ordered float64")
        oks.append(time_bar(ctx, log, X, cls, n_class, a.repeats))
    log("\n## 2. time shares of the new entry (ICIKT_FLAG_TIMING)")
    shares = []
    for name, cls, n_class in layouts:
        log(f"  S = {S}, n = {n}, {name}")
        shares.append(time_shares(ctx, log, X, cls, n_class, a.repeats))
    epilogue_alone(ctx, log, X, a.repeats)
    name, cls, n_class = layouts[1]
    log(f"  S = {S}, n = {n}, {name}, every pass re-reading the kept plane")
    reread = time_shares(ctx, log, X, cls, n_class, a.repeats, spec="medlds=0")
    log(f"  re-reading the kept plane in every pass costs {reread[2] - shares[1][2]:+.2f} ms of epilogue time per call against "
        f"keys staged in LDS once")
    log(f"  the small-class layout: {layouts[2][0]} spends {shares[2][2]:.2f} ms under the epilogue timer, "
        f"{shares[2][2] - shares[0][2]:+.2f} ms against one class")
    log("\n# the new entry not slower than the old route: "
        + ", ".join(f"{name} " + ("YES" if ok else "NO") for (name, _c, _k), ok in zip(layouts, oks)))
    ctx.close()


if __name__ == "__main__":
    main()
