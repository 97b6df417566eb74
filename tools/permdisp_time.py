"""What the PERMDISP entry costs, on one MI355X, every leg in one process on the same card.

Shape: S = 4 096, n = 2 000, F-ordered float64, 999 permutations; three layouts of the classes, class-sorted:
2 classes of 2 048, 16 of 256 and 2 048 of 2.  Per layout:

  1. the two routes, alternating call by call, median of --repeats calls after 2 warm-up calls each:
       (a) the old route: Context.matrix over all pairs, then (1 - raw)^2, the S x C table by one matrix product, the
           within-class sums and the squared distances to the centroids in numpy, in doubles -- what a user writes
           today without a PCoA (--old-repeats calls after --old-warm: a call takes tens of seconds, so fewer may be
           asked for, and the log says how many were made);
       (b) Context.permdisp.
  2. with ICIKT_FLAG_TIMING, alternating in the same way: Context.permdisp, the yardstick Context.permanova with the
     999 permutations and without any, and a keep-only call, Context.mst(min_raw = +inf): the triangle, the keep and
     one sweep of k_mst_best, which finds nothing.  The library accounts everything behind the pair kernel under
     ICIKT_K_EPILOGUE, so what a leg spends behind the pair kernel is logged as it is (keep + finish), and the
     finishes are compared as differences against the keep-only call:
       k_disp_table - k_mst_best          permdisp less keep-only: what the table costs MORE than one sweep of
                                          k_mst_best, which has the same geometry and no bins (the kernel alone is in
                                          a kernel trace: profiles/permdisp_trace.log)
       k_pmv_quant + labelling kernels    permanova less keep-only, for the observed labelling alone and with 999
                                          (less that same sweep)
  3. the front end's host stages, timed apart so that nobody takes them for device time: the S own-class distances
     and class means, and the permutation stage (api._permdisp_permute) over the 999 labellings.

    python tools/permdisp_time.py [--repeats 20] [--old-repeats 20] [--out profiles/permdisp_time.log]
    python tools/permdisp_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
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


def old_route(ctx, X, cls, n_class):
    """The full matrices, then the table and the squared distances to the centroids on the host, in doubles:
    (sum of d^2 over the pairs, T [S, C], D2 [S, C])"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    d = 1.0 - out5[1]
    d2 = d * d
    np.fill_diagonal(d2, 0.0)
    onehot = (cls[:, None] == np.arange(n_class)[None, :]).astype(np.float64)
    T = d2 @ onehot
    sizes = onehot.sum(axis=0)
    A = 0.5 * (T * onehot).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        D2 = T / sizes[None, :] - (A / (sizes * sizes))[None, :]
    return float(np.triu(d2, 1).sum()), T, D2


def alternating(ctx, legs):
    """legs: name -> (callable, calls to time, warm-up calls).  One call of each leg in turn, as long as a leg has calls
    left: per leg the wall seconds, the median [prepare, pairs, epilogue] ms per call and the last result."""
    ts = {k: [] for k in legs}
    shares = {k: [] for k in legs}
    out = {}
    rounds = max(w + r for _f, r, w in legs.values())
    for i in range(rounds):
        for name, (fn, r, w) in legs.items():
            if i >= w + r:
                continue
            ctx.reset_timers()
            t0 = time.perf_counter()
            out[name] = fn()
            t1 = time.perf_counter()
            if i >= w:
                ts[name].append(t1 - t0)
                shares[name].append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
    return ts, {k: np.median(np.asarray(v), axis=0) for k, v in shares.items()}, out


def host_stages(log, cls, n_class, perms, T):
    """the front end's host work on the table, in the front end's own functions"""
    t0 = time.perf_counter()
    sizes, _A, X = api._permdisp_centroids(T, cls, n_class)
    z = np.array([api.permdisp_distance(X[i, cls[i]], int(sizes[cls[i]])) for i in range(cls.shape[0])])
    zi, D = api._permdisp_ints(z)
    means = np.zeros(n_class)
    for c in np.flatnonzero(sizes > 0):
        means[c] = float(api.Fraction(sum(zi[i] for i in np.flatnonzero(cls == c)), D * int(sizes[c])))
    obs = api.permdisp_statistic(z, cls, n_class)
    t1 = time.perf_counter()
    _Fs, n_ge, n_undef = api._permdisp_permute(z - means[cls], perms, n_class, obs.F)
    t2 = time.perf_counter()
    log(f"  host: the S own-class distances, class means and F: {(t1 - t0) * 1e3:10.1f} ms (one call)")
    log(f"  host: the permutation stage, {perms.shape[0]} labellings:    {(t2 - t1) * 1e3:10.1f} ms (one call); "
        f"F = {api._as_float(obs.F):.6g}, n_ge = {n_ge}, n_undefined = {n_undef}")


def layout(log, ctx, X, n_class, n_perm, a):
    S = X.shape[1]
    cls = np.repeat(np.arange(n_class, dtype=np.int32), S // n_class)
    perms = api.anosim_permutations(cls, n_perm, seed=7)
    log(f"\n## {n_class} classes of {S // n_class}, class-sorted")
    ts, _sh, out = alternating(ctx, {"old": (lambda: old_route(ctx, X, cls, n_class), a.old_repeats, a.old_warm),
                                    "new": (lambda: ctx.permdisp(X, cls, n_class), a.repeats, 2)})
    log(f"  (a) Context.matrix + numpy   {fmt(stats(ts['old']))}   ({len(ts['old'])} calls after {a.old_warm} warm-up)")
    log(f"  (b) Context.permdisp         {fmt(stats(ts['new']))}   ({len(ts['new'])} calls after 2 warm-up)")
    log(f"  new route {stats(ts['old'])[0] / stats(ts['new'])[0]:.1f}x the old one's speed at the median")
    old, new = out["old"], out["new"]
    got_T = (new[2] / 2 ** 50).astype(np.float64)
    rel_q = abs(new[1] / 2.0 ** 50 - old[0]) / old[0]
    rel_t = float(np.max(np.abs(got_T - old[1]) / np.maximum(old[1], 1e-300)))
    log(f"  (a) in doubles against (b) in fixed point: relative difference of Q {rel_q:.2e}, largest of a cell of the "
        f"table {rel_t:.2e}; values {new[0][0]}, NA pairs {new[0][1]}")
    F = _lib.FLAG_TIMING
    legs = {"permdisp": (lambda: ctx.permdisp(X, cls, n_class, flags=F), a.repeats, 2),
            "permanova": (lambda: ctx.permanova(X, cls, n_class, perms, flags=F), a.repeats, 2),
            "permanova, no permutation": (lambda: ctx.permanova(X, cls, n_class, None, flags=F), a.repeats, 2),
            "keep only (mst, +inf)": (lambda: ctx.mst(X, min_raw=float("inf"), flags=F), a.repeats, 2)}
    ts, sh, _out = alternating(ctx, legs)
    for name in legs:
        log(f"  {name:28s} {fmt(stats(ts[name]))}   ms per call: copies + pre-pass {sh[name][0]:8.2f}, pair kernel "
            f"{sh[name][1]:8.2f}, everything behind it {sh[name][2]:8.2f}")
    keep = sh["keep only (mst, +inf)"][2]
    disp, pmv0, pmv = sh["permdisp"][2] - keep, sh["permanova, no permutation"][2] - keep, sh["permanova"][2] - keep
    log(f"  behind the pair kernel (keep + finish): permdisp {sh['permdisp'][2]:.3f} ms, permanova "
        f"{sh['permanova, no permutation'][2]:.3f} ms for the observed labelling alone and {sh['permanova'][2]:.3f} ms with "
        f"{n_perm} permutations; ratios {sh['permdisp'][2] / sh['permanova, no permutation'][2]:.3f} and "
        f"{sh['permdisp'][2] / sh['permanova'][2]:.3f}")
    log(f"  less the keep-only call ({keep:.3f} ms, one k_mst_best sweep in it): k_disp_table - k_mst_best {disp:.3f} ms; "
        f"permanova's finish - k_mst_best {pmv0:.3f} ms (observed alone), {pmv:.3f} ms (with the permutations)")
    host_stages(log, cls, n_class, perms, new[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--old-repeats", type=int, default=20)
    ap.add_argument("--old-warm", type=int, default=2)
    ap.add_argument("--layouts", default="2,16,2048", help="numbers of classes, each dividing S")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S, n_perm = (2000, 4096, 999) if not a.quick else (100, 256, 33)
    ctx = _lib.Context(0)
    log("# tools/permdisp_time.py: one process, one card; host clock around calls that end in a stream synchronisation; "
        "seeded generators; the legs alternate call by call" + ("  [--quick: NOT a measurement]" if a.quick else ""))
    log(f"# S = {S}, n = {n} ({S * (S - 1) // 2} pairs), {n_perm} permutations, F-ordered float64")
    X = make(n, S, 1)
    ran = []
    for n_class in (int(v) for v in a.layouts.split(",")):
        if n_class > S or S % n_class:
            log(f"\n## {n_class} classes do not divide S = {S}: not run")
            continue
        layout(log, ctx, X, n_class, n_perm, a)
        ran.append(n_class)
    log(f"\nlayouts run: {ran}; no other shape was run")
    ctx.close()


if __name__ == "__main__":
    main()
