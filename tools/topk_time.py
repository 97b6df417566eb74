"""What the top-k entry costs, on one MI355X, both routes in one process on the same card:

  1. the bar: Context.topk against the route a caller had before it -- Context.matrix, np.argpartition and a sort per
     row on the host -- at S = 4 096, n = 2 000, k = 32, F-ordered float64; the legs alternate;
  2. with ICIKT_FLAG_TIMING, the selection kernels' time (accounted under ICIKT_K_EPILOGUE, beside the pair epilogue)
     next to the pair kernel's, at the shape of (1) and at S = 8 192, n = 64, k = 32, and at the shape of (1) the call
     with the triangle cut into 8 blocks (tkblock) against one block;
  3. the shape the old route cannot serve, S = 32 768, n = 256, k = 32: wall time and the device memory in use during
     the call (torch.cuda.mem_get_info before the call and, polled from a second thread, its low-water mark during
     it), beside the formula of DESIGN.md section 13 and the 5 S^2 x 8 bytes of the full matrices.

    python tools/topk_time.py [--repeats 20] [--big-repeats 3] [--out profiles/topk_time.log]
    python tools/topk_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
"""
import argparse
import os
import sys
import threading
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


def old_route(ctx, X, k):
    """The full matrices, then per row the k largest raw among the other samples (argpartition, then a sort of the k)"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    raw = out5[1].copy()
    np.fill_diagonal(raw, -np.inf)
    raw[np.isnan(raw)] = -np.inf
    S = raw.shape[0]
    kk = min(k, S - 1)
    part = np.argpartition(-raw, kk - 1, axis=1)[:, :kk]
    rows = np.arange(S)[:, None]
    order = np.argsort(-raw[rows, part], axis=1, kind="stable")
    idx = part[rows, order]
    return idx, out5[:, rows, idx]


def time_bar(ctx, log, X, k, repeats, warm=2):
    ta, tb = [], []
    for i in range(warm + repeats):
        t0 = time.perf_counter()
        old = old_route(ctx, X, k)
        t1 = time.perf_counter()
        new = ctx.topk(X, k)
        t2 = time.perf_counter()
        if i >= warm:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
    sa, sb = stats(ta), stats(tb)
    same = bool(np.array_equal(old[1][1], new[1][1][:, :old[0].shape[1]]))   # (the raw values picked; indices may differ among equal raw)
    log(f"  (a) Context.matrix + argpartition + sort per row: {fmt(sa)}")
    log(f"  (b) Context.topk:                                 {fmt(sb)}   raw of the picks {'equal' if same else 'DIFFERS'}")
    log(f"  new route {sa[0] / sb[0]:.2f}x the old one's speed at the median: {'NOT SLOWER' if sb[0] <= sa[0] else 'SLOWER'}")
    return sb[0] <= sa[0]


def time_shares(ctx, log, X, k, repeats, spec=None, warm=2):
    """wall time and, per call, ms under ICIKT_K_PREPARE / _PAIRS / _EPILOGUE (the selection kernels are in the last)"""
    ctx.debug_set_plan(spec)
    ts, shares = [], []
    for i in range(warm + repeats):
        ctx.reset_timers()
        t0 = time.perf_counter()
        ctx.topk(X, k, flags=_lib.FLAG_TIMING)
        t1 = time.perf_counter()
        if i >= warm:
            ts.append(t1 - t0)
            shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    ctx.debug_set_plan(None)
    med = np.median(np.asarray(shares), axis=0)
    launches = ctx.kernel_ms(_lib.K_EPILOGUE)[1]
    log(f"  {str(spec or 'default blocks'):16s} {fmt(stats(ts))}; per call: copies + pre-pass {med[0]:8.2f} ms, pair kernel "
        f"{med[1]:8.2f} ms, pair epilogue + selection {med[2]:8.2f} ms ({launches} timed epilogue spans in the last call)")
    return med


def epilogue_alone(ctx, log, X, repeats, warm=2):
    """the pair epilogue without any selection (Context.pairs with timing): what to take off the figure above"""
    es = []
    for i in range(warm + repeats):
        ctx.reset_timers()
        ctx.pairs(X, flags=_lib.FLAG_TIMING, want_counts=False)
        if i >= warm:
            es.append(ctx.kernel_ms(_lib.K_EPILOGUE)[0])
    log(f"  pair epilogue alone (Context.pairs, same matrix): median {np.median(es):8.2f} ms per call")


def big_shape(ctx, log, n, S, k, repeats):
    import torch
    X = make(n, S, 7)
    torch.cuda.synchronize()
    free0, total = torch.cuda.mem_get_info()
    low = [free0]
    stop = threading.Event()

    def poll():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.02)

    th = threading.Thread(target=poll, daemon=True)
    th.start()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = ctx.topk(X, k)
        ts.append(time.perf_counter() - t0)
    stop.set()
    th.join()
    P = S * (S - 1) // 2
    block = min(P, 1 << 24)
    n_pad, np2 = (n + 63) // 64 * 64, 1 << max(1, (n - 1).bit_length())
    formula = 1.125 * (S * (47 * n_pad + 4096) + min(S, (1 << 30) // (12 * np2)) * 12 * np2 + 132 * S * k + 76 * block)
    log(f"  wall time {fmt(stats(ts))} over {repeats} call(s); {P} pairs, {P / (np.median(ts) * 1e9):.3f}e9 pairs/s")
    log(f"  device memory free before the call {free0 / 2**30:.2f} GiB of {total / 2**30:.2f}; low-water mark during the calls "
        f"{low[0] / 2**30:.2f} GiB: {(free0 - low[0]) / 2**30:.2f} GiB in use by the call")
    log(f"  DESIGN section 13's formula for this shape: {formula / 2**30:.2f} GiB; the five full matrices would take "
        f"{5 * S * S * 8 / 2**30:.1f} GiB on the device and again on the host")
    log(f"  every sample has {int(res[2].min())} .. {int(res[2].max())} partners; max_taumax {res[3]:.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--big-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    bar, short, big = (2000, 4096, 32), (64, 8192, 32), (256, 32768, 32)
    if a.quick:
        bar, short, big = (200, 256, 8), (32, 384, 8), (32, 700, 8)
    ctx = _lib.Context(0)
    log(f"# tools/topk_time.py: median of {a.repeats} calls per leg after 2 warm-up calls (section 3: {a.big_repeats}), one "
        f"process, one card; host clock around calls that end in a stream synchronisation; seeded generators"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    n, S, k = bar
    X = make(n, S, 1)
    log(f"\n## 1. the bar: S = {S}, n = {n}, k = {k}, F-ordered float64")
    ok = time_bar(ctx, log, X, k, a.repeats)
    log(f"\n## 2. time shares (ICIKT_FLAG_TIMING) and block cutting")
    log(f"  S = {S}, n = {n}, k = {k}")
    time_shares(ctx, log, X, k, a.repeats)
    P = S * (S - 1) // 2
    time_shares(ctx, log, X, k, a.repeats, spec=f"tkblock={P // 8 + S}")
    epilogue_alone(ctx, log, X, a.repeats)
    del X
    n, S, k = short
    X = make(n, S, 2)
    log(f"  S = {S}, n = {n}, k = {k}")
    time_shares(ctx, log, X, k, a.repeats)
    epilogue_alone(ctx, log, X, max(3, a.repeats // 4))
    del X
    n, S, k = big
    log(f"\n## 3. the shape the old route cannot serve: S = {S}, n = {n}, k = {k}")
    big_shape(ctx, log, n, S, k, a.big_repeats)
    log("\n# the new entry not slower than the old route at the bar: " + ("YES" if ok else "NO"))
    ctx.close()


if __name__ == "__main__":
    main()
