"""K0 (the per-column pre-pass) alone on the c4 and c3 matrices and longer / shorter columns: device-resident timing
(development aid).  Arguments, in this order, all optional:
  --no-network   time a variant build without the sort's compare-exchanges (-DICIKT_K0_NO_NETWORK, built beside the
                 library; its results are wrong): what the pre-pass takes without its sort;
  a debug plan   e.g. k0=1 (the 256-thread shape);
  config names   c4 c3 c2 ...: bench.py's matrices of those configurations instead of the built-in shapes.
ICIKT_LIB names another build of the library (A/B against a parent commit)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from icikendalltau_amd import _lib
from bench import CONFIGS, make_matrix, workload_matrix
args = sys.argv[1:]
if args[:1] == ["--no-network"]:
    del args[0]
    _lib.LIB_PATH = _lib.build(extra_flags=["-DICIKT_K0_NO_NETWORK"], out=os.path.join(os.path.dirname(_lib.LIB_PATH), "libicikt_hip_k0_no_network.so"))
plan = args.pop(0) if args and "=" in args[0] else None
if args:
    mats = ((c, workload_matrix(c, dict(CONFIGS[c]))) for c in args)
else:
    mats = (("", make_matrix(n, S, na, seed)) for (n, S, na, seed) in ((10000, 1024, 1000, 4), (10000, 256, 500, 3), (50000, 512, 1000, 5), (6887, 96, 300, 2), (3000, 1024, 100, 6), (20000, 512, 500, 7)))
for name, X in mats:
    n, S = X.shape
    ctx = _lib.Context(0)
    if plan:
        ctx.debug_set_plan(plan)     # e.g. k0=1: the 256-thread shape
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    ts = []
    for _ in range(6):
        ctx.reset_timers(); ctx.prepare_dev(dX.data_ptr(), n, S, n, _lib.FLAG_TIMING); ctx.sync()
        ts.append(ctx.kernel_ms(_lib.K_PREPARE)[0])
    print(*([name] if name else []), n, S, "K0 ms", " ".join("%.3f" % t for t in ts), flush=True)
    ctx.close()
