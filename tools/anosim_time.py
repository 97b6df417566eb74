"""What the ANOSIM entry costs, on one MI355X, both routes in one process on the same card:

  1. S = 4 096, n = 2 000, 16 classes of 256, 999 permutations, F-ordered float64:
       (a) Context.matrix over all pairs, then the checker's algorithm vectorised in numpy on the host -- the ranks by
           one sort and two searches, W2 and nW of every labelling as a masked sum over all pairs (median of 3: a call
           takes tens of seconds);
       (b) Context.anosim (median of --repeats);
  2. with ICIKT_FLAG_TIMING the time shares of (b).  The library accounts everything behind the pair kernel under
     ICIKT_K_EPILOGUE, so the split is made of differences between calls:
       pair kernel                       ICIKT_K_PAIRS
       epilogue + statistics + keep      ICIKT_K_EPILOGUE of Context.mst(min_raw = +Inf): the same keep, and one round
                                         of k_mst_best that finds nothing
       count + sort + rank + classes     ICIKT_K_EPILOGUE of Context.anosim without permutations, less the line above
                                         (it includes the permutation kernel over the observed labelling alone)
       the permutation kernel            ICIKT_K_EPILOGUE with 999 permutations less without
       label staging + upload            the wall time's difference between the two calls less the kernel's
  3. S = 32 768, n = 256 (5.4e8 pairs), 99 permutations, the new route only, median of 3, with the free device memory
     after the calls (the context keeps its buffers: the low-water mark).

    python tools/anosim_time.py [--repeats 20] [--out profiles/anosim_time.log]
    python tools/anosim_time.py --old-calls 0  # the device legs only (an A/B of two builds: ICIKT_LIB)
    python tools/anosim_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np   # noqa: E402

from icikendalltau_amd import _lib, api   # noqa: E402
from ingest_time import Tee, fmt, stats   # noqa: E402
from medians_time import make   # noqa: E402


def old_route(ctx, X, cls, perms):
    """The full matrices, then ranks and masked sums on the host: (M, w2, nw) of the observed labelling and every permutation"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    S = X.shape[1]
    iu, ju = np.triu_indices(S, k=1)
    v = out5[1][iu, ju]
    ok = ~np.isnan(v)
    iu, ju, v = iu[ok], ju[ok], v[ok] + 0.0
    M = v.shape[0]
    asc = np.sort(v)
    r2 = (2 * M - np.searchsorted(asc, v, "left") - np.searchsorted(asc, v, "right") + 1).astype(np.int64)
    labs = np.vstack([cls[None, :], perms])
    w2 = np.empty(labs.shape[0], dtype=np.int64)
    nw = np.empty(labs.shape[0], dtype=np.int64)
    for q, lab in enumerate(labs):
        same = lab[iu] == lab[ju]
        w2[q] = r2[same].sum()
        nw[q] = np.count_nonzero(same)
    return M, w2, nw


def timed(ctx, fn, repeats, warm):
    """wall seconds and [prepare, pairs, epilogue] ms per call"""
    ts, shares, out = [], [], None
    for i in range(warm + repeats):
        ctx.reset_timers()
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        if i >= warm:
            ts.append(t1 - t0)
            shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    return ts, np.median(np.asarray(shares), axis=0), out


def free_gb():
    import torch
    free, total = torch.cuda.mem_get_info()
    return free / 2 ** 30, total / 2 ** 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--old-calls", type=int, default=3, help="calls of route (a); 0: the device legs only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S, n_class, n_perm = (2000, 4096, 16, 999) if not a.quick else (100, 256, 4, 33)
    big_n, big_S, big_perm = (256, 32768, 99) if not a.quick else (32, 1024, 9)
    ctx = _lib.Context(0)
    log(f"# tools/anosim_time.py: one process, one card; host clock around calls that end in a stream synchronisation; "
        f"seeded generators" + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    cls = np.repeat(np.arange(n_class, dtype=np.int32), S // n_class)
    perms = api.anosim_permutations(cls, n_perm, seed=7)
    P = S * (S - 1) // 2
    T = _lib.FLAG_TIMING

    log(f"\n## 1. S = {S}, n = {n} ({P} pairs), {n_class} classes of {S // n_class}, {n_perm} permutations, F-ordered float64")
    ta, old = [], None
    for _ in range(a.old_calls):
        t0 = time.perf_counter()
        old = old_route(ctx, X, cls, perms)
        ta.append(time.perf_counter() - t0)
        log(f"  (a) one call: {ta[-1] * 1e3:10.1f} ms")
    tb, sh_full, new = timed(ctx, lambda: ctx.anosim(X, cls, n_class, perms, flags=T), a.repeats, 2)
    sb = stats(tb)
    same = "route (a) was not run"
    if old is not None:
        equal = old[0] == new[0][0] and np.array_equal(old[1], new[1]) and np.array_equal(old[2], new[2])
        same = f"M, W2, nW of all {1 + n_perm} labellings {'equal' if equal else 'DIFFER'}"
        log(f"  (a) Context.matrix + numpy ranks and masked sums ({a.old_calls} calls, no warm-up): {fmt(stats(ta))}")
    log(f"  (b) Context.anosim ({a.repeats} calls after 2 warm-up calls):               {fmt(sb)}   "
        f"{same}; n_ge {new[3]}, n_undefined {new[4]}")
    if old is not None:
        log(f"  new route {stats(ta)[0] / sb[0]:.1f}x the old one's speed at the median")

    log("\n## 2. time shares of (b), ms per call (medians; ICIKT_FLAG_TIMING)")
    t0p, sh_none, _o = timed(ctx, lambda: ctx.anosim(X, cls, n_class, None, flags=T), a.repeats, 2)
    _t, sh_keep, _o = timed(ctx, lambda: ctx.mst(X, float("inf"), flags=T), a.repeats, 2)
    wall_full, wall_none = stats(tb)[0], stats(t0p)[0]
    perm_ms = sh_full[2] - sh_none[2]
    log(f"  copies + pre-pass                                {sh_full[0]:8.2f}")
    log(f"  pair kernel                                      {sh_full[1]:8.2f}")
    log(f"  epilogue + statistics + keep (from Context.mst)  {sh_keep[2]:8.2f}")
    log(f"  count + sort + rank + classes + observed sums    {sh_none[2] - sh_keep[2]:8.2f}")
    log(f"  permutation kernel, {n_perm} permutations            {perm_ms:8.2f}")
    log(f"  label staging + upload (wall difference less the kernel's)  {wall_full - wall_none - perm_ms:8.2f}")
    log(f"  wall: {wall_full:.2f} with {n_perm} permutations, {wall_none:.2f} without")
    log(f"  the permutation kernel against the pair kernel: {perm_ms:.2f} ms against {sh_full[1]:.2f} ms")

    log(f"\n## 3. S = {big_S}, n = {big_n} ({big_S * (big_S - 1) // 2} pairs), {big_perm} permutations, the new route only, median of 3")
    Xb = make(big_n, big_S, 7)
    clsb = np.repeat(np.arange(n_class, dtype=np.int32), big_S // n_class)
    permsb = api.anosim_permutations(clsb, big_perm, seed=7)
    before = free_gb()
    tbig, sh_big, outb = timed(ctx, lambda: ctx.anosim(Xb, clsb, n_class, permsb, flags=T), 3, 1)
    after = free_gb()
    log(f"  Context.anosim: {fmt(stats(tbig))}; per call: copies + pre-pass {sh_big[0]:8.2f} ms, pair kernel {sh_big[1]:8.2f} ms, "
        f"everything behind it {sh_big[2]:8.2f} ms; M {outb[0][0]}, n_ge {outb[3]}")
    log(f"  free device memory: {before[0]:.1f} GB before, {after[0]:.1f} GB after the calls (of {after[1]:.1f} GB): "
        f"{before[0] - after[0]:.1f} GB held by the context")
    ctx.close()


if __name__ == "__main__":
    main()
