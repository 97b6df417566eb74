"""The cases of the device-resident path on a caller's stream (tests/test_stream_cases_host.py checks them with the
oracle alone, tests/test_gpu_caller_stream.py runs them).  Plain numpy: nothing here touches a device.

A case is a column length and a kind of data.  It holds two matrices of the same shape and NaN rate from different
seeds: the TRUE one, whose answers the CPU oracle gives, and a DECOY.  The decoy is valid data: a library that reads its
input too early, or a result too late, computes wrong numbers and never touches memory it should not.  The test tells
the two apart only if every pair's tau differs between them, and tells a buffer the library wrote from one it left
alone by the SENTINEL, which no reference value may equal.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

S = 8
PAIRS = S * (S - 1) // 2                   # 28, in combn order
IU, JU = (a.astype(np.int32) for a in np.triu_indices(S, k=1))
SENTINEL = -7.0
NAN_RATE = 0.08
MAX_FEATURES = 65535                       # ICIKT_MAX_FEATURES: longer columns run the plain 32-bit path, exact integers

# column length -> the launch family or the edge it stands for (csrc/icikt_k1plan.h: plan_k1; icikt_pipeline.cpp: matrix_tied, run_counts)
LENGTHS = {
    40: "short columns, half-wave kernels",
    700: "short columns, half-wave kernels",
    7168: "half-wave kernels of 4 words per lane, no column-statistics read-back",
    10000: "the c4 family",
    14272: "the last length without the column-statistics read-back (k1_half_items < 9)",
    14273: "the first length with the read-back",
    20000: "the 15 200 - 30 656 range, where the read-back picks the kernel family",
    33000: "long columns, whole-wave kernels",
    70000: "k1_wide, which clears d_task_ctr before its launch",
}
ALL_KINDS_AT = (700, 10000, 70000)         # the lengths every stream kind runs at; the others run on the side stream
VARIANTS = ("continuous", "tied")

Case = namedtuple("Case", "n variant")
CASES = tuple(Case(n, v) for n in LENGTHS for v in VARIANTS)


def case_id(case):
    return f"{case.n}-{case.variant}"


def _matrix(n, variant, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, S))
    if variant == "tied":
        X[:, 1::2] = np.round(X[:, 1::2] * 3.0) / 3.0       # every other column in thirds: long tie groups
    X[rng.random((n, S)) < NAN_RATE] = np.nan
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X


@lru_cache(maxsize=None)
def true_matrix(case):
    """[n, S] float64, column-major"""
    return _matrix(case.n, case.variant, 1000 + case.n)


@lru_cache(maxsize=None)
def decoy_matrix(case):
    return _matrix(case.n, case.variant, 5000 + case.n)


def as_float32(X):
    """The values a float32 source of X carries, as float64 (what icikt_convert_dev writes)."""
    Y = np.asfortranarray(X.astype(np.float32).astype(np.float64))
    Y.setflags(write=False)
    return Y


def oracle_answers(X):
    """{perspective: (out4 [28, 4], counts [28, 12], reasons [28])} of the CPU oracle over all pairs of X.  Columns
    past MAX_FEATURES run in exact integer arithmetic in the library (ICIKT_FLAG_EXACT_INT64 is implied there), so the
    oracle does too."""
    from oracle import oracle as O
    compat = X.shape[0] <= MAX_FEATURES
    return {p: O.ici_pairs(X, IU, JU, p, int32_compat=compat) for p in ("global", "local")}


@lru_cache(maxsize=None)
def reference(case):
    return oracle_answers(true_matrix(case))


@lru_cache(maxsize=None)
def decoy_reference(case):
    return oracle_answers(decoy_matrix(case))


def combn_blocks(k=3):
    """k consecutive blocks [begin, end) of the 28 pairs, of unequal length"""
    cuts = np.linspace(0, PAIRS, k + 1).round().astype(int)
    cuts[1] += 1
    return [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


def shuffled_pairs():
    """the 28 pairs in a shuffled order: (permutation, pi, pj)"""
    perm = np.random.default_rng(28).permutation(PAIRS)
    return perm, IU[perm].copy(), JU[perm].copy()


def rank_ranges(world=3):
    """The column ranges of a `world`-rank split of the S columns (an even number of columns per rank: the rec table
    interleaves column pairs) and the columns the prepared state is allocated for."""
    per = 2 * -(-S // (2 * world))
    return [(min(S, r * per), min(S, (r + 1) * per)) for r in range(world)], per * world
