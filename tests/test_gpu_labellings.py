"""The labellings of icikt_anosim_* and icikt_permanova_* through the one driver they share (select_labellings,
csrc/icikt_capi_select.cpp): both entries run through the same test bodies, each against its own brute-force checker
(tests/anosim_checker.py, tests/permanova_checker.py, through the helpers of test_gpu_anosim.py and
test_gpu_permanova.py, which share their references with those modules) with every integer EQUAL.

The data are 65 continuous columns of 40 rows in five unequal classes.  What is varied is what the driver decides: the
number of labellings around one and two groups of 16, the batch (anoperms) around a group, the size of the one label
plane both entries now keep in the context, and a refusal that arrives while a batch is in flight."""
import numpy as np
import pytest

from icikendalltau_amd import _lib
from tests import test_gpu_anosim as ano
from tests import test_gpu_permanova as pmv
from tests.test_gpu_medians import _continuous

pytestmark = pytest.mark.gpu

ENTRIES = {"anosim": ano, "permanova": pmv}
N = 40


def _classes(S):
    """five classes of unequal size; three samples: three of the five declared classes"""
    return ano._unequal5(S) if S >= 10 else (np.array([0, 4, 4], dtype=np.int32)[:S], 5)


def _check(ctx, entry, S, n_perm):
    cls, n_class = _classes(S)
    return ENTRIES[entry]._run(ctx, ("cont", S, N), _continuous(S, N), cls, n_class, n_perm, "u5")


@pytest.mark.parametrize("anoperms", [1, 15, 16, 17])
@pytest.mark.parametrize("n_perm", [14, 15, 16, 31, 32])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_batch_edges(plan_ctx, entry, n_perm, anoperms):
    """1 + n_perm labellings around one group of 16 and around two, in batches of one, of a group less one, of a group
    and of a group and one"""
    plan_ctx.debug_set_plan(f"anoperms={anoperms}")
    got, _ref = _check(plan_ctx, entry, 65, n_perm)
    assert len(got[2]) == 1 + n_perm


def test_one_label_plane_for_both_entries(hip_ctx):
    """the plane is the context's: anosim at S = 65, permanova at twice that, anosim at S = 3, permanova at S = 65 again --
    it grows and is reused larger than a call needs, across the entries"""
    for entry, S in (("anosim", 65), ("permanova", 130), ("anosim", 3), ("permanova", 65)):
        _check(hip_ctx, entry, S, 33)


def _raw_call(ctx, entry, X, cls, n_class, perms, outs):
    """the entry's f64 call on caller-filled output arrays: (return code, message)"""
    L = _lib.lib()
    n, S = X.shape
    fn = {"anosim": L.icikt_anosim_f64, "permanova": L.icikt_permanova_f64}[entry]
    rc = fn(ctx._h, _lib._ptr(X), n, S, n, None, 0, 1, 0, 0, 0, _lib._ptr(cls), n_class, _lib._ptr(perms), perms.shape[0],
            *(_lib._ptr(a) for a in outs), None, None)
    return rc, (L.icikt_last_error(ctx._h) or b"").decode()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_refusal_with_a_batch_in_flight(plan_ctx, entry):
    """34 labellings in batches of 16 and a bad label in row 20, labelling 21: it is met while the first batch's kernels
    run.  The call fails with the entry's message, no output array is written, and the context's next call is right."""
    S, n_perm = 65, 33
    X = np.asfortranarray(_continuous(S, N))
    cls, n_class = _classes(S)
    perms = np.ascontiguousarray(ENTRIES[entry].documented_permutations(cls, n_perm, 7), dtype=np.int32)
    perms[20, 64] = n_class
    n_lab = 1 + n_perm
    sizes = {"anosim": (2, n_lab, n_lab, 1, 1, n_class, n_class),             # n_pairs, w2, nw, n_ge, n_undefined, class_w2, class_nw
             "permanova": (2, 2, n_lab * n_class, n_lab * n_class)}[entry]    # n_pairs, q_total, bins_lo, bins_hi
    outs = [np.full(k, -9, dtype=np.int64) for k in sizes]
    plan_ctx.debug_set_plan("anoperms=16")
    rc, msg = _raw_call(plan_ctx, entry, X, cls, n_class, perms, outs)
    assert rc == -1 and msg == f"{entry}: perm_cls[20][64] = 5 is outside 0 .. n_class - 1 (n_class = 5)", (rc, msg)
    assert all(np.all(a == -9) for a in outs)
    assert plan_ctx.num_pairs() == -1
    _check(plan_ctx, entry, S, n_perm)
