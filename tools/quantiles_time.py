"""What the quantiles entry costs, on one MI355X, both routes in one process on the same card:

  1. the bar: Context.quantiles against the route a caller had before it -- Context.matrix over all pairs, then
     np.quantile and np.histogram over the triangle of raw (per group) on the host -- at S = 4 096, n = 2 000, F-ordered
     float64, probs (0.5, 0.9, 0.99, 0.999), 200 bins, for (a) one group and (b) 16 classes of 256 samples (three
     groups); the legs alternate;
  2. with ICIKT_FLAG_TIMING, the new entry's time under ICIKT_K_PREPARE (copies + pre-pass), ICIKT_K_PAIRS (the pair
     kernel) and ICIKT_K_EPILOGUE (pair epilogue + statistics + fold + select) at both layouts, the same call cut into
     8 blocks and with probs=() (no kept plane, no select), and the pair epilogue alone: fold + select is the
     difference;
  3. S = 32 768, n = 256: 5.4e8 pairs, where the old route cannot run (five matrices of 8.6 GB each).

    python tools/quantiles_time.py [--repeats 20] [--out profiles/quantiles_time.log]
    python tools/quantiles_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
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

PROBS = (0.5, 0.9, 0.99, 0.999)


def make(n, S, seed):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X


def old_route(ctx, X, cls, breaks, tri):
    """The full matrices, then per group np.quantile and np.histogram over the triangle of raw"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    raw = out5[1][tri]
    groups = [raw] if cls is None else [raw, raw[cls[tri[0]] == cls[tri[1]]], raw[cls[tri[0]] != cls[tri[1]]]]
    q, h = [], []
    for g in groups:
        g = g[~np.isnan(g)]
        q.append(np.quantile(g, PROBS, method="linear") if g.size else np.full(len(PROBS), np.nan))
        h.append(np.histogram(g, bins=breaks)[0])
    return np.asarray(q), np.asarray(h)


def time_bar(ctx, log, X, cls, n_class, breaks, repeats, warm=2):
    tri = np.triu_indices(X.shape[1], k=1)
    ta, tb = [], []
    for i in range(warm + repeats):
        t0 = time.perf_counter()
        old_q, old_h = old_route(ctx, X, cls, breaks, tri)
        t1 = time.perf_counter()
        new = ctx.quantiles(X, PROBS, breaks, cls, n_class)
        t2 = time.perf_counter()
        if i >= warm:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
    sa, sb = stats(ta), stats(tb)
    same_h = bool(np.array_equal(old_h, new[4]))
    dq = float(np.max(np.abs(old_q - new[0][1])))
    log(f"  (a) Context.matrix + np.quantile + np.histogram per group: {fmt(sa)}")
    log(f"  (b) Context.quantiles:                                     {fmt(sb)}   histogram "
        f"{'equal' if same_h else 'DIFFERS'}, quantile_raw within {dq:.1e} of np.quantile")
    log(f"  new route {sa[0] / sb[0]:.2f}x the old one's speed at the median: {'NOT SLOWER' if sb[0] <= sa[0] else 'SLOWER'}")
    return sb[0] <= sa[0]


def time_shares(ctx, log, X, cls, n_class, breaks, repeats, probs=PROBS, spec=None, label=None, warm=2):
    """wall time and, per call, ms under ICIKT_K_PREPARE / _PAIRS / _EPILOGUE (fold and select are in the last)"""
    ctx.debug_set_plan(spec)
    ts, shares = [], []
    for i in range(warm + repeats):
        ctx.reset_timers()
        t0 = time.perf_counter()
        ctx.quantiles(X, probs, breaks, cls, n_class, flags=_lib.FLAG_TIMING)
        t1 = time.perf_counter()
        if i >= warm:
            ts.append(t1 - t0)
            shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    ctx.debug_set_plan(None)
    med = np.median(np.asarray(shares), axis=0)
    log(f"  {str(label or spec or 'default'):22s} {fmt(stats(ts))}; per call: copies + pre-pass {med[0]:8.2f} ms, pair kernel "
        f"{med[1]:8.2f} ms, pair epilogue + statistics + fold + select {med[2]:8.2f} ms")
    return med


def epilogue_alone(ctx, log, X, repeats, warm=2):
    """the pair epilogue without statistics, fold or select (Context.pairs with timing): what to take off the figure above"""
    es = []
    for i in range(warm + repeats):
        ctx.reset_timers()
        ctx.pairs(X, flags=_lib.FLAG_TIMING, want_counts=False)
        if i >= warm:
            es.append(ctx.kernel_ms(_lib.K_EPILOGUE)[0])
    med = float(np.median(es))
    log(f"  pair epilogue alone (Context.pairs, all pairs of the same matrix): median {med:8.2f} ms per call")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    ap.add_argument("--no-large", action="store_true", help="skip the S = 32 768 leg")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S, per = (2000, 4096, 256) if not a.quick else (100, 256, 16)
    breaks = np.linspace(-1.0, 1.0, 201)
    ctx = _lib.Context(0)
    log(f"# tools/quantiles_time.py: median of {a.repeats} calls per leg after 2 warm-up calls, one process, one card; host "
        f"clock around calls that end in a stream synchronisation; seeded generators; probs {PROBS}, 200 bins over [-1, 1]"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    many = (np.arange(S) // per).astype(np.int32)
    n_many = S // per
    P = S * (S - 1) // 2
    oks = []
    for name, cls, n_class in (("one group", None, 1), (f"{n_many} classes of {per}: three groups", many, n_many)):
        log(f"\n## 1. the bar: S = {S}, n = {n}, {name} ({P} pairs), F-ordered float64")
        oks.append(time_bar(ctx, log, X, cls, n_class, breaks, a.repeats))
    log("\n## 2. time shares of the new entry (ICIKT_FLAG_TIMING)")
    log(f"  S = {S}, n = {n}, one group")
    full = time_shares(ctx, log, X, None, 1, breaks, a.repeats)
    cut = time_shares(ctx, log, X, None, 1, breaks, a.repeats, spec=f"tkblock={P // 8 + S}")
    hist = time_shares(ctx, log, X, None, 1, breaks, a.repeats, probs=(), label="probs=() (no select)")
    log(f"  S = {S}, n = {n}, {n_many} classes of {per}: three groups")
    full3 = time_shares(ctx, log, X, many, n_many, breaks, a.repeats)
    hist3 = time_shares(ctx, log, X, many, n_many, breaks, a.repeats, probs=(), label="probs=() (no select)")
    epi = epilogue_alone(ctx, log, X, a.repeats)
    log(f"  fold + select = the epilogue share less the pair epilogue alone: one group {full[2] - epi:.2f} ms (fold without "
        f"keys {hist[2] - epi:.2f} ms, 8 blocks {cut[2] - epi:.2f} ms), three groups {full3[2] - epi:.2f} ms (fold without keys "
        f"{hist3[2] - epi:.2f} ms); the pair epilogue alone is {epi:.2f} ms")
    if not a.no_large:
        nL, SL = (256, 32768) if not a.quick else (32, 1024)
        log(f"\n## 3. S = {SL}, n = {nL}: {SL * (SL - 1) // 2} pairs, median of 3 calls after 1 warm-up call (the old route cannot "
            f"run: five S x S matrices)")
        XL = make(nL, SL, 2)
        time_shares(ctx, log, XL, None, 1, breaks, 3, warm=1)
        time_shares(ctx, log, XL, None, 1, breaks, 3, probs=(), label="probs=() (no select)", warm=1)
        manyL = (np.arange(SL) // per).astype(np.int32)
        time_shares(ctx, log, XL, manyL, SL // per, breaks, 3, label=f"{SL // per} classes of {per}", warm=1)
    log("\n# the new entry not slower than the old route: one group " + ("YES" if oks[0] else "NO") + ", three groups "
        + ("YES" if oks[1] else "NO"))
    ctx.close()


if __name__ == "__main__":
    main()
