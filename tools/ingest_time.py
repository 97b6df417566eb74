"""What a caller's natural matrix costs on the way in: for C-ordered float64 / float32 / int32 and
F-ordered float32 / float64 inputs, (a) what every call did before the view existed -- np.asfortranarray(X,
dtype=float64) plus the _f64 entry, timed together -- against (b) the *_in entry on the matrix where it lies; the two
legs alternate in one process.  Then k_ingest alone (HIP events around icikt_convert_dev) with its achieved bytes/s
beside a device-to-device hipMemcpyAsync of the float64 matrix, and, with --parent-lib, the _f64 entry of this build
against the same entry of a build of the parent commit on the F-ordered float64 matrix.

    python tools/ingest_time.py [--repeats 20] [--parent-lib path/to/parent/libicikt_hip.so] [--out profiles/ingest_time.log]
    python tools/ingest_time.py --quick        # tiny shapes: a rehearsal of the script, not a measurement
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np   # noqa: E402

from icikendalltau_amd import _lib   # noqa: E402

GNA = (np.nan, np.inf, 0)


class Tee:
    def __init__(self, path):
        self.f = open(path, "w") if path else None

    def __call__(self, *a):
        line = " ".join(str(x) for x in a)
        print(line, flush=True)
        if self.f:
            self.f.write(line + "\n")
            self.f.flush()


def make_inputs(n, S, seed):
    """One set of values float32 and int32 hold exactly, in the five layouts"""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 4000, size=(n, S)).astype(np.int32)
    q[rng.random((n, S)) < 0.08] = 0                     # global_na holds 0: the missing cells of every input
    return {
        "C float64": np.ascontiguousarray(q, dtype=np.float64),
        "C float32": np.ascontiguousarray(q, dtype=np.float32),
        "C int32": q,
        "F float32": np.asfortranarray(q, dtype=np.float32),
        "F float64": np.asfortranarray(q, dtype=np.float64),
    }


def stats(ts):
    return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def fmt(st):
    return f"median {st[0]:9.2f} ms  (min {st[1]:9.2f}, max {st[2]:9.2f})"


def entry_call(ctx, entry, X, cls):
    if entry == "pairs":
        return ctx.pairs(X, perspective="global", want_counts=False)[0]
    t, s, ex, _m = ctx.censor_counts(X, GNA, cls, 3)
    return np.concatenate([t, s, [ex]])


def time_legs(ctx, entry, X, cls, repeats, warm=2):
    """(a) asfortranarray + _f64 entry, (b) the *_in entry on X; alternating.  Every call ends in the entry's own stream
    synchronisation, so the host clock holds the whole call."""
    ta, tb, ra, rb = [], [], None, None
    for k in range(warm + repeats):
        ctx.f64_entries = True
        t0 = time.perf_counter()
        ra = entry_call(ctx, entry, X, cls)      # (_lib.Context._entry: np.asfortranarray(X, dtype=float64), then icikt_*_f64)
        t1 = time.perf_counter()
        ctx.f64_entries = False
        t2 = time.perf_counter()
        rb = entry_call(ctx, entry, X, cls)
        t3 = time.perf_counter()
        if k >= warm:
            ta.append(t1 - t0)
            tb.append(t3 - t2)
    return stats(ta), stats(tb), bool(np.array_equal(ra, rb, equal_nan=True))


def hip_runtime():
    """The HIP runtime this process has loaded already (torch's), for a plain hipMemcpyAsync"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def time_kernel(ctx, log, n, S, repeats):
    """k_ingest alone: HIP events on the context's stream around `repeats` icikt_convert_dev calls, and the D2D copy"""
    import torch
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    try:
        dst = torch.empty((S, n), dtype=torch.float64, device="cuda")
        src64 = torch.rand((S, n), dtype=torch.float64, device="cuda")

        def timed(fn):
            torch.cuda.synchronize()                  # (the buffers were filled on torch's default stream)
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(repeats):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / repeats      # ms per call

        ms = timed(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src64.data_ptr(), 8 * n * S, 3, stream.cuda_stream))
        yard = 2 * 8 * n * S / (ms * 1e-3)
        log(f"  yardstick  hipMemcpyAsync D2D of 8 n S = {8 * n * S / 1e6:.1f} MB: {ms:8.4f} ms per call, "
            f"{yard / 1e12:.3f} TB/s (read + written)")
        for label, tdt, code, order in (("C float64", torch.float64, _lib.DTYPE_F64, _lib.ORDER_ROW),
                                        ("C float32", torch.float32, _lib.DTYPE_F32, _lib.ORDER_ROW),
                                        ("C int32", torch.int32, _lib.DTYPE_I32, _lib.ORDER_ROW),
                                        ("F float32", torch.float32, _lib.DTYPE_F32, _lib.ORDER_COL)):
            shape = (n, S) if order == _lib.ORDER_ROW else (S, n)
            src = (torch.rand(shape, device="cuda") * 1000).to(tdt)
            ld = shape[1]
            ms = timed(lambda: ctx.convert_dev(src.data_ptr(), code, order, n, S, ld, dst.data_ptr(), n))
            nbytes = n * S * (src.element_size() + 8)
            rate = nbytes / (ms * 1e-3)
            log(f"  k_ingest   {label:10s} {n} x {S}: {ms:8.4f} ms per call (HIP events, {repeats} calls), "
                f"{nbytes / 1e6:.1f} MB read + written, {rate / 1e12:.3f} TB/s = {100 * rate / yard:.0f} % of the D2D copy's rate")
            del src
    finally:
        ctx.use_own_stream()


class RawLib:
    """The _f64 entries of any build of the library (the parent commit's has no *_in entry), bound by hand"""

    def __init__(self, path):
        import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
        L = ctypes.CDLL(path)
        vp, i64, ci, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32
        L.icikt_ctx_create.argtypes = [ci, ctypes.POINTER(vp)]
        L.icikt_ctx_destroy.argtypes = [vp]
        L.icikt_ctx_destroy.restype = None
        L.icikt_pairs_f64.argtypes = [vp, vp, i64, i64, i64, vp, vp, i64, ci, ci, ci, u32, vp, vp, vp]
        L.icikt_censor_counts_f64.argtypes = [vp, vp, i64, i64, i64, vp, ci, vp, ci, u32, vp, vp, vp, vp]
        self.L, self.h = L, vp()
        if L.icikt_ctx_create(0, ctypes.byref(self.h)) != 0:
            raise RuntimeError(f"{path}: icikt_ctx_create failed")

    def call(self, entry, X, cls, out):
        n, S = X.shape
        p = lambda a: a.ctypes.data   # noqa: E731
        if entry == "pairs":
            rc = self.L.icikt_pairs_f64(self.h, p(X), n, S, n, None, None, 0, 1, 0, 0, 0, p(out["out4"]), None, p(out["rsn"]))
        else:
            gna = np.array(GNA, dtype=np.float64)
            rc = self.L.icikt_censor_counts_f64(self.h, p(X), n, S, n, p(gna), 3, p(cls), 3, 0, p(out["tr"]), p(out["su"]),
                                                p(out["ex"]), None)
        if rc != 0:
            raise RuntimeError(f"{entry}: code {rc}")

    def close(self):
        self.L.icikt_ctx_destroy(self.h)


def time_against_parent(log, parent_path, entry, X, cls, repeats, warm=2):
    n, S = X.shape
    P = S * (S - 1) // 2
    out = {"out4": np.empty((P, 4)), "rsn": np.empty(P, dtype=np.int32), "tr": np.zeros(3, dtype=np.int64),
           "su": np.zeros(3, dtype=np.int64), "ex": np.zeros(1, dtype=np.int64)}
    libs = {"parent": RawLib(parent_path), "this build": RawLib(_lib.LIB_PATH)}
    ts = {k: [] for k in libs}
    for k in range(warm + repeats):
        for name, lib in (list(libs.items())[::-1] if k & 1 else libs.items()):   # (alternating which build goes first)
            t0 = time.perf_counter()
            lib.call(entry, X, cls, out)
            t1 = time.perf_counter()
            if k >= warm:
                ts[name].append(t1 - t0)
    for lib in libs.values():
        lib.close()
    sp, sn = stats(ts["parent"]), stats(ts["this build"])
    log(f"  icikt_{entry}_f64, F float64 {n} x {S}: parent     {fmt(sp)}")
    log(f"  icikt_{entry}_f64, F float64 {n} x {S}: this build {fmt(sn)}")
    level = abs(sn[0] - sp[0]) <= (sp[2] - sp[1])
    log(f"  statement 2: medians {sn[0] - sp[0]:+.2f} ms apart, the parent's own min-max spread {sp[2] - sp[1]:.2f} ms: "
        f"{'LEVEL' if level else 'NOT LEVEL'}")


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
    log(f"# tools/ingest_time.py: {a.repeats} repeats per leg after 2 warm-up calls, legs alternating in one process; host "
        f"clock around calls that end in a stream synchronisation" + ("  [--quick: NOT a measurement]" if a.quick else ""))
    for entry, n, S in shapes:
        log(f"\n## {n} x {S} through Context.{entry}")
        inputs = make_inputs(n, S, n + S)
        cls = (np.arange(S) % 3).astype(np.int32)
        res = {}
        for label, X in inputs.items():
            sa, sb, same = time_legs(ctx, entry, X, cls, a.repeats)
            res[label] = (sa, sb)
            log(f"  {label:10s} (a) asfortranarray + _f64 entry: {fmt(sa)}")
            log(f"  {label:10s} (b) the _in entry on the view:  {fmt(sb)}   results {'equal' if same else 'DIFFER'}")
            if label != "F float64":
                gap, spread = sa[0] - sb[0], (sa[2] - sa[1]) + (sb[2] - sb[1])
                log(f"  statement 1, {label}: (b) is {gap:+.2f} ms faster at the median, the two min-max spreads together "
                    f"{spread:.2f} ms: {'HOLDS' if gap > spread else 'DOES NOT HOLD'}")
        time_kernel(ctx, log, n, S, a.repeats)
        if a.parent_lib:
            time_against_parent(log, a.parent_lib, entry, inputs["F float64"], cls, a.repeats)
        else:
            log("  statement 2: no --parent-lib given: not measured")
        cb, fb, f32b = res["C float64"][1], res["F float64"][1], res["F float32"][1]
        log(f"  statement 3: C float64 (b) sits {cb[0] - fb[0]:+.2f} ms above F float64 (b) at the median; the F-ordered leg's "
            f"spread is {fb[2] - fb[1]:.2f} ms (k_ingest's time: the C float64 line above)")
        log(f"  statement 4: F float32 (b) {f32b[0]:.2f} ms against F float64 (b) {fb[0]:.2f} ms at the median: "
            f"{'HOLDS (not slower)' if f32b[0] <= fb[0] + (fb[2] - fb[1]) else 'DOES NOT HOLD'}")
    ctx.close()


if __name__ == "__main__":
    main()
