"""What the padjust entry costs, on one MI355X, both routes in one process on the same card:

  1. Context.padjust against the route a caller had before it -- Context.matrix over all pairs, then the adjustment of
     the triangle of pvalue in numpy on the host (sort, cumulative minimum, counts per alpha) -- at S = 4 096, n = 2 000,
     F-ordered float64, BH, alphas (0.01, 0.05); the legs alternate;
  2. with ICIKT_FLAG_TIMING, the new entry's time under ICIKT_K_PREPARE (copies + pre-pass), ICIKT_K_PAIRS (the pair
     kernel) and ICIKT_K_EPILOGUE (pair epilogue + statistics + fold + sort + adjust + table), per method, the same call
     cut into 8 blocks, and the pair epilogue alone: fold + sort + adjust is the difference.

    python tools/padjust_time.py [--repeats 20] [--out profiles/padjust_time.log]
    python tools/padjust_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
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

ALPHAS = (0.01, 0.05)


def make(n, S, seed):
    """a shared factor under the noise, so that a part of the pairs is rejected, and 8 % missing cells"""
    rng = np.random.default_rng(seed)
    load = rng.uniform(0.0, 0.5, S)
    X = np.asfortranarray(rng.standard_normal(n)[:, None] * load[None, :] + rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X


def old_route(ctx, X, tri):
    """The full matrices, then BH over the triangle of pvalue on the host"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    p = out5[2][tri]
    p = np.sort(p[~np.isnan(p)])
    m = p.shape[0]
    adj = np.minimum(1.0, np.minimum.accumulate(((float(m) / np.arange(1, m + 1, dtype=np.float64)) * p)[::-1])[::-1])
    n_rej = [int(np.searchsorted(adj, a, side="right")) for a in ALPHAS]
    return m, n_rej, [p[k - 1] if k else np.nan for k in n_rej]


def time_bar(ctx, log, X, repeats, warm=2):
    tri = np.triu_indices(X.shape[1], k=1)
    ta, tb = [], []
    for i in range(warm + repeats):
        t0 = time.perf_counter()
        old = old_route(ctx, X, tri)
        t1 = time.perf_counter()
        new = ctx.padjust(X, "BH", ALPHAS, 0)
        t2 = time.perf_counter()
        if i >= warm:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
    sa, sb = stats(ta), stats(tb)
    same = old[0] == new[0][0] and old[1] == new[1].tolist() and \
        np.array_equal(np.asarray(old[2]).view(np.uint64), new[2].view(np.uint64))
    log(f"  (a) Context.matrix + numpy BH over the triangle: {fmt(sa)}")
    log(f"  (b) Context.padjust:                             {fmt(sb)}   m = {new[0][0]}, n_rejected {new[1].tolist()}: "
        f"counts and cut-offs {'equal' if same else 'DIFFER'}")
    log(f"  new route {sa[0] / sb[0]:.2f}x the old one's speed at the median: {'NOT SLOWER' if sb[0] <= sa[0] else 'SLOWER'}")
    return sb[0] <= sa[0]


def time_shares(ctx, log, X, method, repeats, max_table=0, spec=None, label=None, warm=2):
    """wall time and, per call, ms under ICIKT_K_PREPARE / _PAIRS / _EPILOGUE (fold, sort, adjust, table: the last)"""
    ctx.debug_set_plan(spec)
    ts, shares = [], []
    for i in range(warm + repeats):
        ctx.reset_timers()
        t0 = time.perf_counter()
        ctx.padjust(X, method, ALPHAS, max_table, flags=_lib.FLAG_TIMING)
        t1 = time.perf_counter()
        if i >= warm:
            ts.append(t1 - t0)
            shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    ctx.debug_set_plan(None)
    med = np.median(np.asarray(shares), axis=0)
    log(f"  {str(label or method):28s} {fmt(stats(ts))}; per call: copies + pre-pass {med[0]:8.2f} ms, pair kernel "
        f"{med[1]:8.2f} ms, pair epilogue + statistics + fold + sort + adjust + table {med[2]:8.2f} ms")
    return med


def epilogue_alone(ctx, log, X, repeats, warm=2):
    """the pair epilogue without statistics or fold (Context.pairs with timing): what to take off the figure above"""
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
    a = ap.parse_args()
    log = Tee(a.out)
    n, S = (2000, 4096) if not a.quick else (100, 256)
    ctx = _lib.Context(0)
    log(f"# tools/padjust_time.py: median of {a.repeats} calls per leg after 2 warm-up calls, one process, one card; host "
        f"clock around calls that end in a stream synchronisation; seeded generators; alphas {ALPHAS}"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    P = S * (S - 1) // 2
    log(f"\n## 1. both routes: S = {S}, n = {n} ({P} pairs), F-ordered float64, BH")
    ok = time_bar(ctx, log, X, a.repeats)
    log("\n## 2. time shares of the new entry (ICIKT_FLAG_TIMING)")
    full = {m: time_shares(ctx, log, X, m, a.repeats) for m in ("BH", "holm", "hochberg", "bonferroni")}
    table = time_shares(ctx, log, X, "BH", a.repeats, max_table=P, label="BH, max_table = all pairs")
    cut = time_shares(ctx, log, X, "BH", a.repeats, spec=f"tkblock={P // 8 + S}", label=f"BH, tkblock={P // 8 + S}")
    epi = epilogue_alone(ctx, log, X, a.repeats)
    log(f"  fold + sort + adjust = the epilogue share less the pair epilogue alone: BH {full['BH'][2] - epi:.2f} ms (with the "
        f"whole table {table[2] - epi:.2f} ms, 8 blocks {cut[2] - epi:.2f} ms), holm {full['holm'][2] - epi:.2f} ms, hochberg "
        f"{full['hochberg'][2] - epi:.2f} ms, bonferroni {full['bonferroni'][2] - epi:.2f} ms; the pair kernel is "
        f"{full['BH'][1]:.2f} ms, the pair epilogue alone {epi:.2f} ms")
    log("\n# the new entry not slower than the old route: " + ("YES" if ok else "NO") + "; fold + sort + adjust "
        + ("ABOVE" if full['BH'][2] - epi > full['BH'][1] else "below") + " the pair kernel's time")
    ctx.close()


if __name__ == "__main__":
    main()
