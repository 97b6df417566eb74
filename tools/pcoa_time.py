"""What the PCoA entry costs, on one MI355X, every leg in one process on the same card.

Shape: S = 4 096, n = 2 000, F-ordered float64, k = 10, tol = 1e-8, the default basis (128 columns).  The data are
twelve groups of samples, each a noisy copy of its group's profile, with 8 % missing cells: the picture an ordination
is drawn for, with the k axes asked for clear of the bulk.  (The unstructured data of the other tools, whose spectrum
has no gap at all, run the new route alone, and the log says whether it converged.)

  1. the two routes, alternating call by call, median of --repeats calls after 2 warm-up calls each:
       (a) the old route: Context.matrix over all pairs, then (1 - raw)^2, the double centring and numpy.linalg.eigh of
           the S x S table on the host, the 10 largest pairs taken from it;
       (b) Context.pcoa.
  2. with ICIKT_FLAG_TIMING: Context.pcoa's copies + pre-pass, pair kernel and everything behind it (the keep and every
     kernel of the entry, its small mid-call downloads excluded), with n_basis and n_apply.
  3. one k_pcoa_apply (icikt_pcoa_apply_dev) on a table of the same size with b = 10, 16, 32 and 64 columns, as bytes of
     G over time, beside a device-to-device copy of G (which reads AND writes those bytes): --inner launches queued back
     to back between two waits, the median of --repeats such groups.

    python tools/pcoa_time.py [--repeats 20] [--out profiles/pcoa_time.log]
    python tools/pcoa_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
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
from medians_time import make   # noqa: E402
from permdisp_time import alternating   # noqa: E402


GROUPS = 12   # more groups than k: the k largest eigenvalues stand clear of the bulk, as the axes one plots do


def make_groups(n, S, seed):
    rng = np.random.default_rng(seed)
    profiles = rng.standard_normal((n, GROUPS))
    X = np.asfortranarray(profiles[:, np.arange(S) % GROUPS] + 0.6 * rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    return X


def old_route(ctx, X, k):
    """The full matrices, then the centring and the whole spectrum on the host: (eigenvalues [k], vectors [S, k])"""
    out5, _keep, _rc = ctx.matrix(X, None, want_keep=False)
    d = 1.0 - out5[1]
    e = d * d
    np.fill_diagonal(e, 0.0)
    m = e.mean(axis=1)
    G = -0.5 * (e - m[:, None] - m[None, :] + m.mean())
    w, V = np.linalg.eigh(G)
    return w[::-1][:k], V[:, ::-1][:, :k]


def apply_leg(log, ctx, S, repeats, inner):
    import torch
    rng = np.random.default_rng(3)
    G = torch.from_numpy(rng.standard_normal((S, S))).cuda()
    G2 = torch.empty_like(G)
    V = torch.from_numpy(rng.standard_normal((64, S))).cuda()
    W = torch.empty_like(V)
    torch.cuda.synchronize()
    nbytes = G.numel() * 8

    def group(fn, wait):
        ts = []
        for r in range(repeats + 2):
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            wait()
            if r >= 2:
                ts.append((time.perf_counter() - t0) / inner)
        return ts

    log(f"\n## one application of G ({nbytes / 1e6:.1f} MB), {inner} launches between two waits, per launch")
    ts = group(lambda: G2.copy_(G), torch.cuda.synchronize)
    med = stats(ts)[0]
    log(f"  device-to-device copy of G   {fmt(stats(ts))}   {nbytes / med / 1e6:8.1f} GB/s read (and as much written)")
    for b in (10, 16, 32, 64):
        ts = group(lambda: ctx.pcoa_apply_dev(G.data_ptr(), V.data_ptr(), S, b, W.data_ptr()), ctx.sync)
        med = stats(ts)[0]
        log(f"  k_pcoa_apply, b = {b:2d}         {fmt(stats(ts))}   {nbytes / med / 1e6:8.1f} GB/s of G read, "
            f"{2.0 * S * S * b / med / 1e9:8.2f} TFLOP/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--old-repeats", type=int, default=20)
    ap.add_argument("--old-warm", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, S, k = (2000, 4096, 10) if not a.quick else (100, 300, 10)
    ctx = _lib.Context(0)
    log("# tools/pcoa_time.py: one process, one card; host clock around calls that end in a stream synchronisation; "
        "seeded generators; the legs alternate call by call" + ("  [--quick: NOT a measurement]" if a.quick else ""))
    log(f"# S = {S}, n = {n} ({S * (S - 1) // 2} pairs), k = {k}, tol = 1e-8, default max_basis, F-ordered float64")
    X = make_groups(n, S, 1)
    log("\n## twelve groups of samples (noisy copies of three profiles), 8 % missing cells")
    ts, _sh, out = alternating(ctx, {"old": (lambda: old_route(ctx, X, k), a.old_repeats, a.old_warm),
                                    "new": (lambda: ctx.pcoa(X, k=k), a.repeats, 2)})
    log(f"  (a) Context.matrix + numpy centring + eigh   {fmt(stats(ts['old']))}   ({len(ts['old'])} calls after {a.old_warm} warm-up)")
    log(f"  (b) Context.pcoa                             {fmt(stats(ts['new']))}   ({len(ts['new'])} calls after 2 warm-up)")
    log(f"  new route {stats(ts['old'])[0] / stats(ts['new'])[0]:.1f}x the old one's speed at the median")
    (w_old, _V_old), new = out["old"], out["new"]
    lam, res, frob = new[3], new[5], new[6]
    log(f"  eigenvalues (b): {np.array2string(lam, precision=6)}")
    log(f"  largest |lambda (a) - lambda (b)| / |G|_F {float(np.abs(w_old - lam).max() / frob):.2e}; largest residual / |G|_F "
        f"{float(res.max() / frob):.2e}; n_basis {new[8]}, n_apply {new[9]}, converged {new[10]}; values {new[0][0]}, NA pairs {new[0][1]}")
    F = _lib.FLAG_TIMING
    for name, data in (("twelve groups", X), ("unstructured (no gap in the spectrum)", make(n, S, 1))):
        ts, sh, out = alternating(ctx, {"pcoa": (lambda: ctx.pcoa(data, k=k, flags=F), a.repeats, 2)})
        r = out["pcoa"]
        log(f"  {name}: Context.pcoa {fmt(stats(ts['pcoa']))}   ms per call: copies + pre-pass {sh['pcoa'][0]:8.2f}, pair kernel "
            f"{sh['pcoa'][1]:8.2f} ({100 * sh['pcoa'][1] / stats(ts['pcoa'])[0]:.0f} % of the call), the keep and the entry's kernels "
            f"{sh['pcoa'][2]:8.2f}; n_basis {r[8]}, n_apply {r[9]}, converged {r[10]}, largest residual / |G|_F {float(r[5].max() / r[6]):.2e}")
    apply_leg(log, ctx, S, a.repeats, a.inner)
    log(f"\nshapes run: S = {S}, n = {n}; no other shape was run (S = 32 768 and S = 65 535 were not run)")
    ctx.close()


if __name__ == "__main__":
    main()
