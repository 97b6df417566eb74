"""What a sparse matrix costs on the way in: for scipy CSC matrices of two densities and two value
types, (a) the only route a sparse matrix had before the *_csc entries -- A.toarray() on the host plus the dense _in
entry, timed together -- against (b) the *_csc entry on the CSC arrays where they lie; the two legs alternate in one
process.  A.toarray() alone is reported beside them.  Then k_scatter_csc alone (the host clock around
icikt_scatter_csc_dev, which ends in a stream synchronisation, on device-resident arrays) with its achieved bytes/s beside
a device-to-device hipMemcpyAsync of the dense float64 matrix, and, with --parent-lib, the dense _f64 entries of this
build against those of a build of the parent commit (tools/ingest_time.py's statement 2).

    python tools/sparse_time.py [--repeats 20] [--parent-lib path/to/parent/libicikt_hip.so] [--out profiles/sparse_time.log]
    python tools/sparse_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np   # noqa: E402
import scipy.sparse as sp   # noqa: E402

from icikendalltau_amd import _lib   # noqa: E402
from ingest_time import GNA, Tee, fmt, hip_runtime, stats, time_against_parent   # noqa: E402


def make_csc(n, S, density, dtype, seed):
    """Count-like values (1 .. 4000, which float32 holds exactly) at `density`, int32 indices, built column by column
    from a seeded generator without ever holding the dense matrix"""
    rng = np.random.default_rng(seed)
    counts = rng.binomial(n, density, size=S)
    indptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    indices = np.empty(indptr[-1], dtype=np.int32)
    for j in range(S):
        indices[indptr[j]:indptr[j + 1]] = np.sort(rng.choice(n, size=counts[j], replace=False))
    data = rng.integers(1, 4000, size=indptr[-1]).astype(dtype)
    return sp.csc_matrix((data, indices, indptr), shape=(n, S))


def entry_call(ctx, entry, X, cls):
    if entry == "pairs":
        return ctx.pairs(X, perspective="global", want_counts=False)[0]
    t, s, ex, _m = ctx.censor_counts(X, GNA, cls, 3)
    return np.concatenate([t, s, [ex]])


def time_legs(ctx, entry, A, cls, repeats, warm=2):
    """(a) A.toarray() + the dense _in entry, (b) the _csc entry on A, alternating; (t) A.toarray() alone, inside (a)"""
    ta, tb, tt, ra, rb = [], [], [], None, None
    for k in range(warm + repeats):
        t0 = time.perf_counter()
        D = A.toarray()
        t1 = time.perf_counter()
        ra = entry_call(ctx, entry, D, cls)
        t2 = time.perf_counter()
        del D
        t3 = time.perf_counter()
        rb = entry_call(ctx, entry, A, cls)
        t4 = time.perf_counter()
        if k >= warm:
            ta.append(t2 - t0)
            tt.append(t1 - t0)
            tb.append(t4 - t3)
    return stats(ta), stats(tb), stats(tt), bool(np.array_equal(ra, rb, equal_nan=True))


def time_kernel(ctx, log, A, repeats):
    """k_scatter_csc alone on device-resident arrays, and the D2D copy of the dense float64 matrix as the yardstick"""
    import ctypes
    import torch
    n, S = A.shape
    stream = torch.cuda.Stream()
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    dst = torch.empty((S, n), dtype=torch.float64, device="cuda")
    src64 = torch.rand((S, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        hip.hipMemcpyAsync(dst.data_ptr(), src64.data_ptr(), 8 * n * S, 3, stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(repeats):
        hip.hipMemcpyAsync(dst.data_ptr(), src64.data_ptr(), 8 * n * S, 3, stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / repeats
    yard = 2 * 8 * n * S / (ms * 1e-3)
    log(f"  yardstick      hipMemcpyAsync D2D of 8 n S = {8 * n * S / 1e6:.1f} MB: {ms:8.4f} ms per call, "
        f"{yard / 1e12:.3f} TB/s (read + written)")
    del src64
    v = _lib.csc_view(A)
    d = [torch.from_numpy(a).cuda() for a in (v.data, v.indices, v.indptr)]
    torch.cuda.synchronize()
    code, itype = _lib.DTYPES[v.data.dtype], _lib.INDEX_TYPES[v.indices.dtype]
    ts = []
    for k in range(3 + repeats):
        t0 = time.perf_counter()
        ctx.scatter_csc_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), code, itype, 0.0, n, S, dst.data_ptr(), n)
        t1 = time.perf_counter()
        if k >= 3:
            ts.append(t1 - t0)
    st = stats(ts)
    nbytes = 8 * n * S + v.data.size * (v.data.itemsize + v.indices.itemsize)
    rate = nbytes / (st[0] * 1e-3)
    log(f"  k_scatter_csc  {v.data.dtype}/{v.indices.dtype} {n} x {S}, {v.data.size} entries: {fmt(st)} per "
        f"icikt_scatter_csc_dev call (host clock: the read-back of indptr, the kernel, the record's way back and one stream "
        f"synchronisation), {nbytes / 1e6:.1f} MB written + read, {rate / 1e12:.3f} TB/s = {100 * rate / yard:.0f} % of the "
        f"D2D copy's rate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: rehearses the script, measures nothing")
    a = ap.parse_args()
    log = Tee(a.out)
    shapes = [("pairs", 10000, 1024), ("censor_counts", 50000, 2048)]
    if a.quick:
        shapes = [("pairs", 500, 64), ("censor_counts", 2000, 96)]
    ctx = _lib.Context(0)
    log(f"# tools/sparse_time.py: median of {a.repeats} calls per leg after 2 warm-up calls, legs alternating in one process; "
        f"host clock around calls that end in a stream synchronisation; seeded generators"
        + ("  [--quick: NOT a measurement]" if a.quick else ""))
    lost = []
    for entry, n, S in shapes:
        log(f"\n## {n} x {S} through Context.{entry}")
        cls = (np.arange(S) % 3).astype(np.int32)
        for density in (0.10, 0.01):
            for dtype in (np.float32, np.float64):
                A = make_csc(n, S, density, dtype, seed=n + S)
                label = f"d = {density:.2f} {np.dtype(dtype).name}/int32"
                dense_b, csc_b = np.dtype(dtype).itemsize * n * S, A.nnz * (A.data.itemsize + 4) + 4 * (S + 1)
                sa, sb, st, same = time_legs(ctx, entry, A, cls, a.repeats)
                log(f"  {label:22s} bytes across PCIe: dense {dense_b / 1e6:8.1f} MB, CSC {csc_b / 1e6:8.1f} MB ({dense_b / csc_b:.1f}x)")
                log(f"  {label:22s} (t) A.toarray() alone:              {fmt(st)}")
                log(f"  {label:22s} (a) A.toarray() + the _in entry:    {fmt(sa)}")
                log(f"  {label:22s} (b) the _csc entry on the arrays:   {fmt(sb)}   results {'equal' if same else 'DIFFER'}")
                faster = sb[0] < sa[0]
                log(f"  {label:22s} new route {sa[0] / sb[0]:.2f}x the old one's speed at the median: "
                    f"{'FASTER' if faster else 'NOT FASTER'}")
                if not faster:
                    lost.append((entry, label))
                if dtype == np.float32:
                    time_kernel(ctx, log, A, a.repeats)
                del A
        if a.parent_lib:
            rng = np.random.default_rng(n + S)
            q = rng.integers(1, 4000, size=(n, S)).astype(np.float64)
            q[rng.random((n, S)) < 0.08] = 0
            time_against_parent(log, a.parent_lib, entry, np.asfortranarray(q), cls, a.repeats)
        else:
            log("  dense route against the parent build: no --parent-lib given: not measured")
    log("\n# every row faster by the new route: " + ("YES" if not lost else f"NO -- {lost}"))
    ctx.close()


if __name__ == "__main__":
    main()
