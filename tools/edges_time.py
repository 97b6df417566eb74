"""What the threshold entry costs, on one MI355X, both routes in one process on the same card:

  1. the bar: Context.edges against the route a caller had before it -- Context.matrix, then np.nonzero on the upper
     triangle of raw >= min_raw and a gather of the five values -- at S = 4 096, n = 2 000, F-ordered float64, min_raw
     the 99th percentile of the off-diagonal raw; the legs alternate;
  2. with ICIKT_FLAG_TIMING, the time under ICIKT_K_EPILOGUE (the pair epilogue, the statistics and the compaction
     kernels) next to the pair kernel's, for the triangle as one block and cut into 8 blocks (tkblock), beside the pair
     epilogue alone (Context.pairs): the difference is what the compaction adds.

    python tools/edges_time.py [--repeats 20] [--out profiles/edges_time.log]
    python tools/edges_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
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


def old_route(ctx, X, thr):
    """The full matrices, then the upper-triangle cells with raw >= thr (row-major nonzero: combn order) and their values"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero(np.triu(out5[1] >= thr, k=1))
    return i, j, out5[:, i, j]


def time_bar(ctx, log, X, thr, room, repeats, warm=2):
    ta, tb = [], []
    for k in range(warm + repeats):
        t0 = time.perf_counter()
        old = old_route(ctx, X, thr)
        t1 = time.perf_counter()
        new = ctx.edges(X, min_raw=thr, max_edges=room)
        t2 = time.perf_counter()
        if k >= warm:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
    sa, sb = stats(ta), stats(tb)
    same = bool(new[3] == len(old[0]) and np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1])
                and np.array_equal(old[2].view(np.int64), np.ascontiguousarray(new[2]).view(np.int64)))
    log(f"  {new[3]} edges of {X.shape[1] * (X.shape[1] - 1) // 2} pairs; room for {room}")
    log(f"  (a) Context.matrix + np.nonzero on the triangle + gather: {fmt(sa)}")
    log(f"  (b) Context.edges:                                        {fmt(sb)}   lists and values {'equal' if same else 'DIFFER'}")
    log(f"  new route {sa[0] / sb[0]:.2f}x the old one's speed at the median: {'NOT SLOWER' if sb[0] <= sa[0] else 'SLOWER'}")
    return sb[0] <= sa[0], sa[0], sb[0]


def time_shares(ctx, log, X, thr, room, repeats, spec=None, warm=2):
    """wall time and, per call, ms under ICIKT_K_PREPARE / _PAIRS / _EPILOGUE (the compaction kernels are in the last)"""
    ctx.debug_set_plan(spec)
    ts, shares = [], []
    for k in range(warm + repeats):
        ctx.reset_timers()
        t0 = time.perf_counter()
        ctx.edges(X, min_raw=thr, max_edges=room, flags=_lib.FLAG_TIMING)
        t1 = time.perf_counter()
        if k >= warm:
            ts.append(t1 - t0)
            shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    ctx.debug_set_plan(None)
    med = np.median(np.asarray(shares), axis=0)
    spans = ctx.kernel_ms(_lib.K_EPILOGUE)[1]
    log(f"  {str(spec or 'one block'):16s} {fmt(stats(ts))}; per call: copies + pre-pass {med[0]:8.2f} ms, pair kernel "
        f"{med[1]:8.2f} ms, pair epilogue + statistics + compaction {med[2]:8.2f} ms ({spans} timed epilogue spans in the last call)")
    return med


def epilogue_alone(ctx, log, X, repeats, warm=2):
    """the pair epilogue without statistics or compaction (Context.pairs with timing): what to take off the figure above"""
    es = []
    for k in range(warm + repeats):
        ctx.reset_timers()
        ctx.pairs(X, flags=_lib.FLAG_TIMING, want_counts=False)
        if k >= warm:
            es.append(ctx.kernel_ms(_lib.K_EPILOGUE)[0])
    log(f"  pair epilogue alone (Context.pairs, same matrix): median {np.median(es):8.2f} ms per call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S = (200, 256) if a.quick else (2000, 4096)
    ctx = _lib.Context(0)
    log(f"# tools/edges_time.py: median of {a.repeats} calls per leg after 2 warm-up calls, one process, one card; host clock "
        f"around calls that end in a stream synchronisation; seeded generator"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    raw = out5[1][np.triu_indices(S, k=1)]
    thr = float(np.quantile(raw[~np.isnan(raw)], 0.99))
    del out5, raw
    P = S * (S - 1) // 2
    room = min(P, max(2 ** 20, 32 * S))                  # api.ici_kendalltau_edges' first call
    log(f"\n## 1. the bar: S = {S}, n = {n}, F-ordered float64, min_raw = {thr:.6f} (the 99th percentile of raw)")
    ok, _ta, _tb = time_bar(ctx, log, X, thr, room, a.repeats)
    log("\n## 2. time shares (ICIKT_FLAG_TIMING) and block cutting")
    time_shares(ctx, log, X, thr, room, a.repeats)
    time_shares(ctx, log, X, thr, room, a.repeats, spec=f"tkblock={P // 8 + S}")
    epilogue_alone(ctx, log, X, a.repeats)
    log("\n# the new entry not slower than the old route at the bar: " + ("YES" if ok else "NO"))
    ctx.close()


if __name__ == "__main__":
    main()
