"""What the class-medians entry costs, on one MI355X, both routes in one process on the same card:

  1. the bar: Context.class_medians against the route a caller had before it -- Context.matrix over all pairs, then
     np.nanmedian over each class's block of cor on the host -- at S = 4 096, n = 2 000, F-ordered float64, for (a) one
     class and (b) 16 classes of 256 samples; the legs alternate;
  2. with ICIKT_FLAG_TIMING, the new entry's time under ICIKT_K_PREPARE (copies + pre-pass), ICIKT_K_PAIRS (the pair
     kernel) and ICIKT_K_EPILOGUE (pair epilogue + keep + select) at both class layouts, and the pair epilogue alone;
  3. the two select paths at S = 4 096, one class (4 095 partners per sample): keys staged in LDS once (the default)
     against every pass re-reading the kept plane (medlds=0).

    python tools/medians_time.py [--repeats 20] [--out profiles/medians_time.log]
    python tools/medians_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
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


def old_route(ctx, X, cls, n_class):
    """The full matrices, then per class np.nanmedian over the rows of its block of cor and of raw (diagonal out)"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    S = X.shape[1]
    med2 = np.full((2, S), np.nan)
    for k in range(n_class):
        members = np.nonzero(cls == k)[0]
        if len(members) < 2:
            continue
        for q in (0, 1):
            block = out5[q][np.ix_(members, members)]
            np.fill_diagonal(block, np.nan)
            med2[q, members] = np.nanmedian(block, axis=1)
    return med2


def time_bar(ctx, log, X, cls, n_class, repeats, warm=2):
    ta, tb = [], []
    for i in range(warm + repeats):
        t0 = time.perf_counter()
        old = old_route(ctx, X, cls, n_class)
        t1 = time.perf_counter()
        new = ctx.class_medians(X, cls, n_class)
        t2 = time.perf_counter()
        if i >= warm:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
    sa, sb = stats(ta), stats(tb)
    same = bool(np.array_equal(old[1], new[0][1]))   # med_raw (cor is scaled by another maximum when there are several classes)
    log(f"  (a) Context.matrix + np.nanmedian per class block: {fmt(sa)}")
    log(f"  (b) Context.class_medians:                         {fmt(sb)}   med_raw {'equal' if same else 'DIFFERS'}")
    log(f"  new route {sa[0] / sb[0]:.2f}x the old one's speed at the median: {'NOT SLOWER' if sb[0] <= sa[0] else 'SLOWER'}")
    return sb[0] <= sa[0]


def time_shares(ctx, log, X, cls, n_class, repeats, spec=None, warm=2):
    """wall time and, per call, ms under ICIKT_K_PREPARE / _PAIRS / _EPILOGUE (keep and select are in the last)"""
    ctx.debug_set_plan(spec)
    ts, shares = [], []
    for i in range(warm + repeats):
        ctx.reset_timers()
        t0 = time.perf_counter()
        ctx.class_medians(X, cls, n_class, flags=_lib.FLAG_TIMING)
        t1 = time.perf_counter()
        if i >= warm:
            ts.append(t1 - t0)
            shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    ctx.debug_set_plan(None)
    med = np.median(np.asarray(shares), axis=0)
    log(f"  {str(spec or 'default'):10s} {fmt(stats(ts))}; per call: copies + pre-pass {med[0]:8.2f} ms, pair kernel "
        f"{med[1]:8.2f} ms, pair epilogue + keep + select {med[2]:8.2f} ms")
    return med


def epilogue_alone(ctx, log, X, repeats, warm=2):
    """the pair epilogue without keep or select (Context.pairs with timing): what to take off the figure above"""
    es = []
    for i in range(warm + repeats):
        ctx.reset_timers()
        ctx.pairs(X, flags=_lib.FLAG_TIMING, want_counts=False)
        if i >= warm:
            es.append(ctx.kernel_ms(_lib.K_EPILOGUE)[0])
    log(f"  pair epilogue alone (Context.pairs, all pairs of the same matrix): median {np.median(es):8.2f} ms per call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S, per = (2000, 4096, 256) if not a.quick else (100, 256, 16)
    ctx = _lib.Context(0)
    log(f"# tools/medians_time.py: median of {a.repeats} calls per leg after 2 warm-up calls, one process, one card; host "
        f"clock around calls that end in a stream synchronisation; seeded generators"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    one = np.zeros(S, dtype=np.int32)
    many = (np.arange(S) // per).astype(np.int32)
    n_many = S // per
    oks = []
    for name, cls, n_class in (("one class", one, 1), (f"{n_many} classes of {per}", many, n_many)):
        pairs = sum(m * (m - 1) // 2 for m in np.bincount(cls).tolist())
        log(f"\n## 1. the bar: S = {S}, n = {n}, {name} ({pairs} within-class pairs of {S * (S - 1) // 2}), F-ordered float64")
        oks.append(time_bar(ctx, log, X, cls, n_class, a.repeats))
    log("\n## 2. time shares of the new entry (ICIKT_FLAG_TIMING)")
    log(f"  S = {S}, n = {n}, one class")
    time_shares(ctx, log, X, one, 1, a.repeats)
    log(f"  S = {S}, n = {n}, {n_many} classes of {per}")
    time_shares(ctx, log, X, many, n_many, a.repeats)
    epilogue_alone(ctx, log, X, a.repeats)
    log(f"\n## 3. the select paths: S = {S}, n = {n}, one class, {S - 1} partners per sample")
    staged = time_shares(ctx, log, X, one, 1, a.repeats)
    reread = time_shares(ctx, log, X, one, 1, a.repeats, spec="medlds=0")
    log(f"  re-reading the kept plane in every pass costs {reread[2] - staged[2]:+.2f} ms of epilogue time per call against "
        f"keys staged in LDS once")
    log("\n# the new entry not slower than the old route: one class " + ("YES" if oks[0] else "NO") + ", "
        + f"{n_many} classes " + ("YES" if oks[1] else "NO"))
    ctx.close()


if __name__ == "__main__":
    main()
