"""Length and width sweep of the pre-pass (development aid): plan k0=0 (the large shape) against k0=2 (512 threads, two
workgroups per CU), alternated, device-resident timing as tools/k0_time.py takes it.  What icikt_k0plan.h's range was
set from (profiles/k0_two_in_flight.log).  Arguments, both optional: rounds (3), column lengths (comma-separated)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from icikendalltau_amd import _lib
from bench import make_matrix

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
LENS = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [3000, 6000, 10000, 20000, 50000]
WIDTHS = (512, 1024, 2048)
print("# n  S  round  k0=0 mean ms (4 calls)  k0=2 mean ms (4 calls)  ratio   [n/10 smallest values per column missing]", flush=True)
for n in LENS:
    X = make_matrix(n, max(WIDTHS), n // 10, 100 + n)
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    del X
    for S in WIDTHS:
        ctx = _lib.Context(0)
        wins = 0
        for r in range(ROUNDS):
            t = {}
            for plan in ("k0=0", "k0=2"):
                ctx.debug_set_plan(plan)
                ts = []
                for i in range(5):
                    ctx.reset_timers(); ctx.prepare_dev(dX.data_ptr(), n, S, n, _lib.FLAG_TIMING); ctx.sync()
                    ts.append(ctx.kernel_ms(_lib.K_PREPARE)[0])
                t[plan] = (float(np.mean(ts[1:])), ts)
            wins += t["k0=2"][0] < t["k0=0"][0]
            print(n, S, r, "%.4f" % t["k0=0"][0], "%.4f" % t["k0=2"][0], "%.3f" % (t["k0=2"][0] / t["k0=0"][0]),
                  " raw", " ".join("%.3f" % x for x in t["k0=0"][1]), "|", " ".join("%.3f" % x for x in t["k0=2"][1]), flush=True)
        print("## n", n, "S", S, "k0=2 faster in", wins, "of", ROUNDS, "rounds", flush=True)
        ctx.close()
    del dX
