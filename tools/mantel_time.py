"""What the Mantel entry costs, on one MI355X, both routes in one process on the same card:

  1. S = 4 096, n = 2 000, 999 permutations, F-ordered float64, `other` = |t_i - t_j| of a random time per sample, for
     method pearson and method spearman:
       (a) Context.matrix over all pairs, a host copy of the raw plane, then the numpy loop a user writes today: per
           permutation the fancy-indexed S x S table of `other`, its triangle, and one dot product with the centred
           x (median of --old-calls calls: a call takes minutes);
       (b) Context.mantel (median of --repeats after 2 warm-ups);
  2. with ICIKT_FLAG_TIMING the time shares of (b).  The library accounts everything behind the pair kernel under
     ICIKT_K_EPILOGUE, so the split is made of differences between calls:
       pair kernel                       ICIKT_K_PAIRS
       y + keep + x's integers + T_obs   ICIKT_K_EPILOGUE of Context.mantel without permutations
       the y ranking                     that figure for spearman less the same for pearson, less the x ranking, which
                                         is Context.anosim's count + sort + rank (its ICIKT_K_EPILOGUE without
                                         permutations less Context.mst's keep): what is left is y's keys, count, sort,
                                         rank against y's quantisation
       k_mantel_perm                     ICIKT_K_EPILOGUE with 999 permutations less without
       k_anosim_perm                     the same difference of Context.anosim, for the same 999 permutations applied
                                         to 16 classes of 256: the kernel k_mantel_perm started from

    python tools/mantel_time.py [--repeats 20] [--old-calls 3] [--out profiles/mantel_time.log]
    python tools/mantel_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np   # noqa: E402

from icikendalltau_amd import _lib, api   # noqa: E402
from anosim_time import timed   # noqa: E402
from ingest_time import Tee, fmt, stats   # noqa: E402
from medians_time import make   # noqa: E402


def old_route(ctx, X, other_sq, method, perms):
    """The full matrices, then numpy: r of the identity and of every permutation, in doubles"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    S = X.shape[1]
    iu, ju = np.triu_indices(S, k=1)
    x = 1.0 - np.array(out5[1])[iu, ju]
    y = other_sq[iu, ju]
    if method == "spearman":
        from scipy.stats import rankdata
        x, ry = rankdata(x), rankdata(y)
        table = np.zeros((S, S))
        table[iu, ju] = table[ju, iu] = ry
    else:
        table = other_sq
    xc = x - x.mean()
    xn = np.sqrt(np.dot(xc, xc))
    y0 = table[iu, ju]
    yn = np.sqrt(np.dot(y0 - y0.mean(), y0 - y0.mean()))
    r = np.empty(1 + perms.shape[0])
    r[0] = np.dot(xc, y0) / (xn * yn)
    for t, pi in enumerate(perms):
        r[1 + t] = np.dot(xc, table[np.ix_(pi, pi)][iu, ju]) / (xn * yn)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--old-calls", type=int, default=3, help="calls of route (a) per method; 0: the device legs only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S, n_class, n_perm = (2000, 4096, 16, 999) if not a.quick else (100, 256, 4, 33)
    ctx = _lib.Context(0)
    log(f"# tools/mantel_time.py: one process, one card; host clock around calls that end in a stream synchronisation; "
        f"seeded generators" + ("  [--quick: NOT a measurement]" if a.quick else ""))
    X = make(n, S, 1)
    t = np.random.default_rng(3).uniform(0.0, 100.0, size=S)
    other_sq = np.abs(t[:, None] - t[None, :])
    iu, ju = np.triu_indices(S, k=1)
    other = np.ascontiguousarray(other_sq[iu, ju])
    perms = api.mantel_permutations(S, n_perm, seed=7)
    cls = np.repeat(np.arange(n_class, dtype=np.int32), S // n_class)
    P = S * (S - 1) // 2
    T = _lib.FLAG_TIMING
    log(f"\n## 1. S = {S}, n = {n} ({P} pairs), {n_perm} permutations, F-ordered float64, other = |t_i - t_j|")
    full, none = {}, {}
    for method in ("pearson", "spearman"):
        ta, old = [], None
        for _ in range(a.old_calls):
            t0 = time.perf_counter()
            old = old_route(ctx, X, other_sq, method, perms)
            ta.append(time.perf_counter() - t0)
            log(f"  {method:8s} (a) one call: {ta[-1] * 1e3:10.1f} ms")
        tb, sh_full, new = timed(ctx, lambda: ctx.mantel(X, other, method, perms, flags=T), a.repeats, 2)
        t0p, sh_none, _o = timed(ctx, lambda: ctx.mantel(X, other, method, None, flags=T), a.repeats, 2)
        full[method], none[method] = (stats(tb), sh_full), (stats(t0p), sh_none)
        r_new = np.array([api._as_float(api.mantel_statistic(P, v, *new[2])) for v in new[1]])
        same = "route (a) was not run"
        if old is not None:
            same = (f"largest |r(a) - r(b)| over {1 + n_perm} labellings {np.max(np.abs(old - r_new)):.3g}; n_ge in doubles "
                    f"{int(np.sum(old[1:] >= old[0]))}")
            log(f"  {method:8s} (a) Context.matrix + numpy loop ({a.old_calls} calls, no warm-up): {fmt(stats(ta))}")
        log(f"  {method:8s} (b) Context.mantel ({a.repeats} calls after 2 warm-up calls):      {fmt(stats(tb))}   "
            f"r {r_new[0]:.12g}, n_ge {new[3]}, n_le {new[4]}, NA pairs {new[0][1]}; {same}")
        if old is not None:
            log(f"  {method:8s} new route {stats(ta)[0] / stats(tb)[0]:.1f}x the old one's speed at the median")

    log("\n## 2. time shares of (b), ms per call (medians; ICIKT_FLAG_TIMING)")
    labs = cls[perms]                                   # the labellings ANOSIM draws for the same seed
    ts_a, an_full, _o = timed(ctx, lambda: ctx.anosim(X, cls, n_class, labs, flags=T), a.repeats, 2)
    _t, an_none, _o = timed(ctx, lambda: ctx.anosim(X, cls, n_class, None, flags=T), a.repeats, 2)
    _t, sh_keep, _o = timed(ctx, lambda: ctx.mst(X, float("inf"), flags=T), a.repeats, 2)
    x_rank = an_none[2] - sh_keep[2]
    for method in ("pearson", "spearman"):
        (wall_full, sh_full), (wall_none, sh_none) = full[method], none[method]
        perm_ms = sh_full[2] - sh_none[2]
        log(f"  {method}: wall {wall_full[0]:.2f} with {n_perm} permutations, {wall_none[0]:.2f} without")
        log(f"    copies + pre-pass                                {sh_full[0]:8.2f}")
        log(f"    pair kernel                                      {sh_full[1]:8.2f}")
        log(f"    y + keep + x's integers + T_obs (no permutations){sh_none[2]:8.2f}")
        log(f"    k_mantel_perm, {n_perm} permutations               {perm_ms:8.2f}   ({perm_ms / max(sh_full[1], 1e-9) * 100:.1f} % of the pair kernel)")
        log(f"    index staging + upload (wall difference less the kernel's)  {wall_full[0] - wall_none[0] - perm_ms:8.2f}")
    y_rank = (none["spearman"][1][2] - none["pearson"][1][2]) - x_rank
    log(f"  epilogue + statistics + keep (from Context.mst)    {sh_keep[2]:8.2f}")
    log(f"  x ranking: ANOSIM's count + sort + rank + classes  {x_rank:8.2f}")
    log(f"  y ranking: spearman less pearson less the x ranking {y_rank:8.2f}   ({y_rank / max(full['spearman'][1][1], 1e-9) * 100:.1f} % of the pair kernel)")
    log(f"  k_anosim_perm, the same {n_perm} permutations as labellings of {n_class} classes   {an_full[2] - an_none[2]:8.2f}   "
        f"(Context.anosim wall {stats(ts_a)[0]:.2f})")
    ctx.close()


if __name__ == "__main__":
    main()
