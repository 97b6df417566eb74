"""What a reference that stays prepared saves, on one MI355X, all legs in one process on the same
card: batches of Sq = 64 samples against a reference of Sr = 4 096, n = 2 000, k = 32, F-ordered float64 -- section 23's
shape.

  (a) Context.cross: both matrices uploaded and pre-passed with every call (section 23's route);
  (b) Context.prepare_reference: the reference's upload and pre-pass, paid once per reference;
  (c) Context.cross_prepared per batch, top-k only;
  (d) (c) with 16 classes of 256 reference samples: the class table as well;
  (e) Context.class_matrix on the stacked matrix (the queries a 17th class): the old way to (d)'s table, all
      C(Sq + Sr, 2) pairs.

The legs alternate; (a) and (e) run on a context of their own, because every other entry drops a prepared reference.
With ICIKT_FLAG_TIMING, (c)'s and (d)'s time per kernel class: copies + pre-pass, pair kernel, pair epilogue + folds.

    python tools/cross_prepared_time.py [--repeats 20] [--out profiles/cross_prepared_time.log]
    python tools/cross_prepared_time.py --quick       # tiny shapes: a rehearsal of the script, not a measurement
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


def same_bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    n, Sq, Sr, k, C = (200, 8, 256, 8, 4) if a.quick else (2000, 64, 4096, 32, 16)
    warm = 2
    own, kept = _lib.Context(0), _lib.Context(0)
    log(f"# tools/cross_prepared_time.py: median of {a.repeats} calls per leg after {warm} warm-up calls, the legs alternating in "
        f"one process on one card; host clock around calls that end in a stream synchronisation; seeded generators"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    Q, R = make(n, Sq, 1), make(n, Sr, 2)
    X = np.asfortranarray(np.hstack([Q, R]))
    ref_cls = np.repeat(np.arange(C, dtype=np.int32), Sr // C)
    all_cls = np.concatenate([np.full(Sq, C, dtype=np.int32), ref_cls])
    log(f"\n## Sq = {Sq}, Sr = {Sr}, n = {n}, k = {k}, {C} classes of {Sr // C}, F-ordered float64: {Sq * Sr} pairs of the "
        f"rectangle, {(Sq + Sr) * (Sq + Sr - 1) // 2} of the stacked triangle")
    ta, tb, tc, td, te = [], [], [], [], []
    for i in range(warm + a.repeats):
        t0 = time.perf_counter()
        ra = own.cross(Q, R, k, want_matrix=False)
        t1 = time.perf_counter()
        kept.prepare_reference(R, Sq)
        t2 = time.perf_counter()
        rc = kept.cross_prepared(Q, k, want_matrix=False)
        t3 = time.perf_counter()
        rd = kept.cross_prepared(Q, k, False, ref_cls, C)
        t4 = time.perf_counter()
        re = own.class_matrix(X, all_cls, C + 1)
        t5 = time.perf_counter()
        if i >= warm:
            for t, d in ((ta, t1 - t0), (tb, t2 - t1), (tc, t3 - t2), (td, t4 - t3), (te, t5 - t4)):
                t.append(d)
    same_c = np.array_equal(ra[1], rc[1]) and same_bits(ra[2], rc[2]) and ra[4] == rc[4]
    same_d = same_bits(rd[6][1], re[0][1][:Sq, :C]) and np.array_equal(rd[7], re[1][:Sq, :C])
    sa, sb, sc, sd, se = (stats(t) for t in (ta, tb, tc, td, te))
    log(f"  (a) Context.cross, top-k only:                                {fmt(sa)}")
    log(f"  (b) Context.prepare_reference ({Sr} columns, once per reference): {fmt(sb)}")
    log(f"  (c) Context.cross_prepared, top-k only:                       {fmt(sc)}   lists {'equal' if same_c else 'DIFFER'} to (a)'s")
    log(f"  (d) Context.cross_prepared, top-k and the {Sq} x {C} class table:  {fmt(sd)}")
    log(f"  (e) Context.class_matrix on the stacked matrix:               {fmt(se)}   med_raw and n_valid of the query rows "
        f"{'equal' if same_d else 'DIFFER'} to (d)'s")
    log(f"  (c) is {sa[0] / sc[0]:.2f}x leg (a)'s speed at the median; (d) is {se[0] / sd[0]:.2f}x leg (e)'s; "
        f"(b) + m (c) is below m (a) from m = {int(np.floor(sb[0] / max(sa[0] - sc[0], 1e-12))) + 1} batches on"
        if sa[0] > sc[0] else f"  (c) is NOT faster than (a) at the median: {sc[0]:.2f} against {sa[0]:.2f} ms")
    log("\n## per kernel class (ICIKT_FLAG_TIMING), median per call")
    for name, call in (("(a) cross, top-k only", lambda: own.cross(Q, R, k, want_matrix=False, flags=_lib.FLAG_TIMING)),
                       ("(b) prepare_reference", lambda: kept.prepare_reference(R, Sq, flags=_lib.FLAG_TIMING)),
                       ("(c) cross_prepared, top-k only", lambda: kept.cross_prepared(Q, k, want_matrix=False, flags=_lib.FLAG_TIMING)),
                       ("(d) ... and the class table", lambda: kept.cross_prepared(Q, k, False, ref_cls, C, flags=_lib.FLAG_TIMING))):
        ctx = own if name.startswith("(a)") else kept
        shares = []
        for i in range(warm + a.repeats):
            ctx.reset_timers()
            call()
            if i >= warm:
                shares.append([ctx.kernel_ms(q)[0] for q in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)])
        med = np.median(np.asarray(shares), axis=0)
        log(f"  {name:32s} copies + pre-pass {med[0]:8.3f} ms, pair kernel {med[1]:8.3f} ms, pair epilogue + folds {med[2]:8.3f} ms")
    own.close()
    kept.close()


if __name__ == "__main__":
    main()
