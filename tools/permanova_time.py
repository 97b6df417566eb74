"""What the PERMANOVA entry costs, on one MI355X, every leg in one process on the same card:

  1. S = 4 096, n = 2 000, 16 classes of 256, 999 permutations, F-ordered float64:
       (a) the old route: Context.matrix over all pairs, then (1 - raw)^2 and, per labelling, the within-class sums per
           class by a mask and numpy.bincount on the host, in doubles -- what a user writes today (--old-calls calls,
           no warm-up: a call takes the better part of a minute);
       (b) Context.permanova;
       (c) Context.anosim, the yardstick: the same triangle, labels and batches, a rank sum in place of the class sums.
     (b) and (c) alternate, call by call: median of --repeats after 2 warm-up calls each.
  2. with ICIKT_FLAG_TIMING the time shares of (b) and (c).  The library accounts everything behind the pair kernel
     under ICIKT_K_EPILOGUE, so the split is made of differences between calls:
       pair kernel                              ICIKT_K_PAIRS
       everything behind it, no permutation     ICIKT_K_EPILOGUE of the call without permutations (it includes the
                                                labelling kernels over the observed labelling alone)
       the labelling kernels                    ICIKT_K_EPILOGUE with 999 permutations less without: k_pmv_perm and
                                                k_pmv_classes for (b), k_anosim_perm for (c)
     and the ratio of the two entries' labelling kernels from this one run.
  3. the same with 2 classes of 2 048: the class kernel's worst case (every column of a labelling adds to one of two
     bins).  (b) and (c) only.

    python tools/permanova_time.py [--repeats 20] [--out profiles/permanova_time.log]
    python tools/permanova_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
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


def old_route(ctx, X, cls, n_class, perms):
    """The full matrices, then squared dissimilarities and masked per-class sums on the host, in doubles:
    (sum of d^2, [1 + n_perm, n_class] within-class sums)"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    S = X.shape[1]
    iu, ju = np.triu_indices(S, k=1)
    d = 1.0 - out5[1][iu, ju]
    d2 = d * d
    labs = np.vstack([cls[None, :], perms])
    within = np.empty((labs.shape[0], n_class), dtype=np.float64)
    for q, lab in enumerate(labs):
        li = lab[iu]
        same = li == lab[ju]
        within[q] = np.bincount(li[same], weights=d2[same], minlength=n_class)
    return float(d2.sum()), within


def alternating(ctx, legs, repeats, warm):
    """legs: name -> callable.  One call of each leg in turn, warm + repeats rounds: per leg the wall seconds, the
    median [prepare, pairs, epilogue] ms per call and the last result."""
    ts = {k: [] for k in legs}
    shares = {k: [] for k in legs}
    out = {}
    for i in range(warm + repeats):
        for name, fn in legs.items():
            ctx.reset_timers()
            t0 = time.perf_counter()
            out[name] = fn()
            t1 = time.perf_counter()
            if i >= warm:
                ts[name].append(t1 - t0)
                shares[name].append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    return ts, {k: np.median(np.asarray(v), axis=0) for k, v in shares.items()}, out


def device_legs(log, ctx, X, cls, n_class, perms, repeats):
    """(b) and (c) with and without permutations, alternating; logs the walls and the split; returns (b)'s last result"""
    T = _lib.FLAG_TIMING
    n_perm = perms.shape[0]
    legs = {"permanova": lambda: ctx.permanova(X, cls, n_class, perms, flags=T),
            "anosim": lambda: ctx.anosim(X, cls, n_class, perms, flags=T),
            "permanova, no permutation": lambda: ctx.permanova(X, cls, n_class, None, flags=T),
            "anosim, no permutation": lambda: ctx.anosim(X, cls, n_class, None, flags=T)}
    ts, sh, out = alternating(ctx, legs, repeats, 2)
    for name in legs:
        log(f"  {name:28s} {fmt(stats(ts[name]))}   ms per call: copies + pre-pass {sh[name][0]:8.2f}, pair kernel "
            f"{sh[name][1]:8.2f}, everything behind it {sh[name][2]:8.2f}")
    pmv = sh["permanova"][2] - sh["permanova, no permutation"][2]
    ano = sh["anosim"][2] - sh["anosim, no permutation"][2]
    log(f"  the labelling kernels, {n_perm} permutations: permanova (k_pmv_perm + k_pmv_classes) {pmv:.3f} ms, "
        f"anosim (k_anosim_perm) {ano:.3f} ms: ratio {pmv / ano if ano > 0 else float('nan'):.3f}")
    log(f"  per 1 000 labellings: permanova {pmv * 1000 / max(n_perm, 1):.3f} ms, anosim {ano * 1000 / max(n_perm, 1):.3f} ms")
    return out["permanova"], stats(ts["permanova"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--old-calls", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S, n_perm = (2000, 4096, 999) if not a.quick else (100, 256, 33)
    ctx = _lib.Context(0)
    log(f"# tools/permanova_time.py: one process, one card; host clock around calls that end in a stream synchronisation; "
        f"seeded generators; the device legs alternate call by call" + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    P = S * (S - 1) // 2

    n_class = 16
    cls = np.repeat(np.arange(n_class, dtype=np.int32), S // n_class)
    perms = api.anosim_permutations(cls, n_perm, seed=7)
    log(f"\n## 1. S = {S}, n = {n} ({P} pairs), {n_class} classes of {S // n_class}, {n_perm} permutations, F-ordered float64")
    ta, old = [], None
    for _ in range(a.old_calls):
        t0 = time.perf_counter()
        old = old_route(ctx, X, cls, n_class, perms)
        ta.append(time.perf_counter() - t0)
        log(f"  (a) Context.matrix + numpy, one call: {ta[-1] * 1e3:10.1f} ms")
    log("## 2. (b) Context.permanova and (c) Context.anosim, and their split")
    new, sb = device_legs(log, ctx, X, cls, n_class, perms, a.repeats)
    if old is not None:
        got_q = new[1] / 2.0 ** 50
        got_within = (new[2] / 2 ** 50).astype(np.float64)
        rel = max(abs(got_q - old[0]) / old[0], float(np.max(np.abs(got_within - old[1]) / np.maximum(old[1], 1e-300))))
        log(f"  (a) in doubles against (b) in fixed point: largest relative difference of a sum {rel:.2e}; "
            f"values {new[0][0]}, NA pairs {new[0][1]}")
        log(f"  new route {stats(ta)[0] / sb[0]:.1f}x the old one's speed at the median ({len(ta)} call(s) of the old route)")

    n_class = 2
    cls = np.repeat(np.arange(n_class, dtype=np.int32), S // n_class)
    perms = api.anosim_permutations(cls, n_perm, seed=7)
    log(f"\n## 3. the same matrix, {n_class} classes of {S // n_class}, {n_perm} permutations (the old route was not run)")
    device_legs(log, ctx, X, cls, n_class, perms, a.repeats)
    log("\nno other shape was run")
    ctx.close()


if __name__ == "__main__":
    main()
