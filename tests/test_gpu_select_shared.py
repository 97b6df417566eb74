"""The selection entries (icikt_topk_*, icikt_edges_*, icikt_class_medians_*) share one host driver
(csrc/icikt_capi_select.cpp) and one context's buffers: a call must leave nothing behind that the next call, of another
entry or of the matrix entry, could pick up -- the reduction words (d_red), the pair kernel's counts (raw_valid), a combn
range or a pair list.  Every result on a shared context is compared bit for bit with the same call on a fresh one."""
import numpy as np
import pytest

from icikendalltau_amd import _lib

pytestmark = pytest.mark.gpu


def _same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_entries_leave_nothing_behind():
    S, n = 65, 40
    rng = np.random.default_rng(20)
    X = np.asfortranarray(rng.standard_normal((n, S)))
    X[rng.random((n, S)) < 0.08] = np.nan
    X[:, 5] = 1.0                                   # a constant column: its pairs carry a reason code
    total = S * (S - 1) // 2
    cls = (np.arange(S) % 3).astype(np.int32)       # three interleaved classes ...
    cls[S - 1] = 3                                  # ... and a singleton
    calls = {
        "topk": lambda c: c.topk(X, 7),
        "edges": lambda c: c.edges(X, min_raw=0.0, max_edges=total),
        "medians": lambda c: c.class_medians(X),
        "medians_cls": lambda c: c.class_medians(X, cls, 4),
        "matrix": lambda c: c.matrix(X),
    }
    fresh = {}
    for name, call in calls.items():
        ctx = _lib.Context(0)
        try:
            fresh[name] = call(ctx)
        finally:
            ctx.close()
    assert fresh["topk"][4][1:].sum() > 0 and fresh["medians_cls"][3][1:].sum() > 0    # reason_counts are not all zero
    assert 0 < fresh["edges"][3] < total and np.isfinite(fresh["topk"][3])
    assert fresh["medians_cls"][2] <= fresh["medians"][2] == fresh["topk"][3] == fresh["edges"][5]   # max_taumax

    shared = _lib.Context(0)
    try:
        for spec in ("tkblock=1000", None):         # the triangle in several blocks of rows, and in one
            shared.debug_set_plan(spec)
            for order in (("topk", "edges", "medians", "medians_cls"), ("medians_cls", "edges", "medians", "topk")):
                for name in order:
                    assert _same(calls[name](shared), fresh[name]), (spec, order, name)
                    assert _same(calls["matrix"](shared), fresh["matrix"]), (spec, order, name, "matrix")
    finally:
        shared.close()
