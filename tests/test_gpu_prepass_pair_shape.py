"""The third shape of the pre-pass kernel -- 512 threads x 8 elements, two workgroups (two columns) in flight on a CU,
plan key k0 = 2 -- against the large shape (k0 = 0) and the CPU oracle, and the pass behind the one-word sort, which
gathers a position's full key only where its 48-bit prefix equals a neighbour's, on every shape.

Bars as in test_gpu_parity: integer counts and reasons bit-exact against the oracle, the four doubles within 1e-10; the
shapes against each other bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ATOL = 1e-10
LARGE, SMALL, PAIR = 0, 1, 2


def _oracle_pairs(X, pi=None, pj=None):
    from oracle import oracle as O
    if pi is None:
        pi, pj = np.triu_indices(X.shape[1], k=1)
    return O.ici_pairs(X, pi, pj, "global", "two.sided", False, int32_compat=True)


def _equals_oracle(res, oracle):
    out, cnt, rsn = res
    ref, rcnt, rrsn = oracle
    assert np.array_equal(rsn, rrsn), (rsn[:20], rrsn[:20])
    ok = rrsn == 0
    assert np.array_equal(cnt[ok], rcnt[ok][:, :cnt.shape[1]]), "integer counts differ"
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    d = np.nanmax(np.abs(out - ref)) if np.any(~np.isnan(ref)) else 0.0
    assert d <= ATOL, d


def _bit_equal(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))   # doubles by their bits: NaN payloads included


def _column_mix(n, rng, S=6):
    """test_prepass_small_shape's columns: ties at 3 and 200 levels, one-word collisions, 7 % NaN, one column 60 % missing."""
    X = rng.standard_normal((n, S))
    if n > 8:
        X[:, 1] = np.round(X[:, 1] * 3)
        X[:, 2] = np.round(X[:, 2] * 200)
        X[:, 3] = 1.0 + (rng.permutation(n) % 50000) * 2.0 ** -52        # one-word collisions everywhere
        X[rng.random(X.shape) < 0.07] = np.nan
        X[:, 5] = np.where(rng.random(n) < 0.6, np.nan, X[:, 5])
    return X


def _run_shapes(ctx, X, shapes, n_oracle_pairs=None):
    """The matrix under every shape of `shapes`: bit for bit the same, and the oracle's (all pairs, or the first few)."""
    res = {}
    for s in shapes:
        ctx.debug_set_plan({"k0": s})
        res[s] = ctx.pairs(X, perspective="global")
    for s in shapes[1:]:
        _bit_equal(res[shapes[0]], res[s])
    if n_oracle_pairs is None:
        oracle = _oracle_pairs(X)
        for s in shapes:
            _equals_oracle(res[s], oracle)
    else:   # (long columns: the oracle on a few pairs; the shapes are equal bit for bit on all of them)
        pi, pj = np.triu_indices(X.shape[1], k=1)
        oracle = _oracle_pairs(X, pi[:n_oracle_pairs], pj[:n_oracle_pairs])
        for s in shapes:
            _equals_oracle(tuple(a[:n_oracle_pairs] for a in res[s]), oracle)
    return res


# the new tile (4 096), the rec / hirow staging edges (2 n_pad <= 3 TILE, n_pad <= 3 TILE), two full tiles, long columns
@pytest.mark.parametrize("n", [1, 64, 65, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 8193, 12288, 12289, 16385, 30000, 65535])
def test_pair_shape_equals_large_shape(plan_ctx, n):
    X = _column_mix(n, np.random.default_rng(n + 5))
    _run_shapes(plan_ctx, X, (LARGE, PAIR), n_oracle_pairs=None if n <= 20000 else 5)


@pytest.mark.parametrize("n", [9001, 10000])
def test_pair_shape_with_exactly_1000_missing(plan_ctx, n):
    """The benchmark's missingness: the 1 000 smallest values of every column.  10 000 rows are c4's plan under the
    512-thread shape -- 9 000 present values: two full tiles, a 1 024-element sub-tile, one more merge level through the
    scratch; 9 001 rows leave 8 001: two tiles, the second mostly padding."""
    rng = np.random.default_rng(n + 5)
    X = _column_mix(n, rng)
    X[np.isnan(X)] = 0.25                                   # (the mix without its missing cells: ties and collisions stay)
    idx = np.argpartition(X, 1000, axis=0)[:1000]
    np.put_along_axis(X, idx, np.nan, axis=0)
    assert np.all(np.isnan(X).sum(axis=0) == 1000)
    _run_shapes(plan_ctx, X, (LARGE, PAIR))


def test_two_workgroups_on_a_cu(plan_ctx):
    """Three columns per CU of the device: under k0 = 2 two workgroups share a CU -- its LDS, its registers -- and a third
    waits for one of them."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, S = 300, 3 * cus
    rng = np.random.default_rng(300)
    X = rng.standard_normal((n, S))
    X[:, 1::3] = np.round(X[:, 1::3] * 3)
    X[:, 2::5] = 1.0 + (rng.integers(0, 50000, (n, len(range(2, S, 5))))) * 2.0 ** -52
    X[rng.random(X.shape) < 0.07] = np.nan
    pi, pj = (a.astype(np.int32) for a in np.triu_indices(8, k=1))
    res = {}
    for s in (LARGE, PAIR):
        plan_ctx.debug_set_plan({"k0": s})
        res[s] = plan_ctx.pairs(X, pi, pj, "global")
    _bit_equal(res[LARGE], res[PAIR])
    _equals_oracle(res[PAIR], _oracle_pairs(X, pi, pj))
    # every column of the launch, not only the first eight: the last ones against the first
    qi = np.arange(S - 8, S, dtype=np.int32)
    qj = np.arange(8, dtype=np.int32)
    tail = {}
    for s in (LARGE, PAIR):
        plan_ctx.debug_set_plan({"k0": s})
        tail[s] = plan_ctx.pairs(X, qi, qj, "global")
    _bit_equal(tail[LARGE], tail[PAIR])
    _equals_oracle(tail[PAIR], _oracle_pairs(X, qi, qj))


def _prefix_columns(n, rng):
    """Columns for the pass behind the one-word sort.  A value's 48-bit prefix holds the top 36 bits of its mantissa:
    values 2^-30 apart (relatively) differ in it, values 2^-50 apart share it."""
    ulp = 2.0 ** -52
    cols = []
    # 0: every value shares its top 48 bits, distinct low bits in random order: inversions, the three-word pass
    cols.append(1.0 + (rng.permutation(n) % 60000) * ulp)
    # 1: the same with ties among the low bits, negative (keys complemented)
    cols.append(-(3.0 + (rng.integers(0, 5000, n) * 4) * ulp))
    # 2 / 3: only every OTHER neighbour pair collides -- couples (v, v + 2^-50), the couples 2^-30 apart; 2: the lower
    # value of a couple in the lower row (the one-word order is the full order: no second pass, the gathers decide the
    # group starts), 3: in either row (inversions)
    rows = rng.permutation(n)
    base = 1.0 + np.arange((n + 1) // 2) * 2.0 ** -30
    for in_order in (True, False):
        v = np.empty(n)
        a, b = rows[0:2 * (n // 2):2], rows[1:2 * (n // 2):2]
        lo, hi = (np.minimum(a, b), np.maximum(a, b)) if in_order else (a, b)
        v[lo] = base[:n // 2]
        v[hi] = base[:n // 2] + 2.0 ** -50
        if n & 1:
            v[rows[-1]] = base[-1]
        cols.append(v)
    # 4: all-distinct prefixes, every value twice: tie groups of 2 that only the full keys show
    cols.append(rng.permutation(np.repeat(base, 2)[:n]))
    # 5: +-0 and subnormals (test_values_that_differ_only_in_their_low_bits): prefixes all equal
    z = np.where(rng.random(n) < 0.3, 0.0, rng.integers(-2, 3, n) * 2.0 ** -1070)
    z[::97] = -0.0
    cols.append(z)
    # 6: continuous: no prefix repeats, nothing is gathered;  7: 200 levels, every prefix repeats inside a group
    cols.append(rng.standard_normal(n))
    cols.append(np.round(rng.standard_normal(n) * 200))
    return np.asfortranarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("n", [700, 5000, 12000])
def test_full_keys_gathered_only_where_prefixes_repeat(plan_ctx, n, missing):
    """Every shape, columns sorted whole (nothing missing) and present values only (5 % missing: the fill group in front
    of the sorted words)."""
    rng = np.random.default_rng(n + int(missing))
    X = _prefix_columns(n, rng)
    assert X.shape[1] == 8
    s = np.sort(X[:, 2])   # (the couples are what the docstring says)
    assert np.all(np.diff(s) > 0) and np.all(np.diff(s)[0::2] < 2.0 ** -49) and np.all(np.diff(s)[1::2] > 2.0 ** -31)
    if missing:
        X[rng.random(X.shape) < 0.05] = np.nan
    _run_shapes(plan_ctx, X, (LARGE, SMALL, PAIR))
