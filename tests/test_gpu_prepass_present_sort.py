"""The pre-pass sorts only a column's PRESENT values: the missing and excluded rows go straight to the front of the
ascending order (their key, fill = min - 0.1, is below every present value), the present values are compacted by the
missing-row bitset, and what is left over behind the full 8 192-element tiles is sorted as a sub-tile of its own size
(icikt_prepass.hip: sort_pass).  Every case goes through the public pair entry with counts and is compared with the CPU
oracle as tests/test_gpu_parity.py::_check does -- counts bit-exact, doubles within 1e-10 -- and the column order the
pre-pass leaves behind with numpy's stable argsort of the fill-substituted column.  The shapes put the present count
p = n - n_na on both sides of every size at which the sort changes its plan: the sub-tile sizes, one tile, one tile + a
sub-tile, two tiles, two tiles + one value, three tile slots."""
import numpy as np
import pytest

from tests.test_gpu_parity import ATOL, _check

pytestmark = pytest.mark.gpu

TILE = 8192   # elements of the sort tile of columns of more than 4 096 rows (k0_prepare_large8)


def _order(ctx, n, S):
    """The ascending order of every column as the pre-pass left it (PrepView::order holds it descending)."""
    import torch
    ptr, bpc = ctx.prep_arrays()[0]

    class _D:  # zero-copy view of the library's buffer
        __cuda_array_interface__ = {"shape": (bpc * S,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    o = torch.as_tensor(_D(), device="cuda").cpu().numpy().view(np.uint16).reshape(S, -1)
    return o[:, :n][:, ::-1].astype(np.int64)


def _check_with_order(ctx, X):
    res = _check(ctx, X, perspective="global")
    n, S = X.shape
    got = _order(ctx, n, S)
    for c in range(S):
        col = X[:, c].copy()
        if np.all(np.isnan(col)):
            continue   # (no minimum: fill is not a number the column could be compared by)
        col[np.isnan(col)] = np.nanmin(col) - 0.1
        assert np.array_equal(got[c], np.argsort(col, kind="stable")), c
    return res


def _columns(rng, n, S=5):
    X = rng.standard_normal((n, S))
    X[:, 1] = np.round(X[:, 1] * 50)       # many small tie groups
    X[:, 2] = np.round(X[:, 2] * 3)        # a few long ones
    return X


def _drop(rng, X, n_na):
    """n_na missing rows per column, other rows in every column; column 3: its n_na smallest values."""
    n, S = X.shape
    for c in range(S):
        rows = np.argsort(X[:, c], kind="stable")[:n_na] if c == 3 else rng.permutation(n)[:n_na]
        X[rows, c] = np.nan
    return X


# p on both sides of: the 4 096-element sub-tile, one tile, a tile + a 1 024-element sub-tile, two tiles
@pytest.mark.parametrize("p", [4095, 4096, 4097, TILE - 1, TILE, TILE + 1, TILE + 1023, TILE + 1024, TILE + 1025,
                               2 * TILE - 1, 2 * TILE, 2 * TILE + 1])
def test_present_count_around_tile_edges(hip_ctx, p):
    rng = np.random.default_rng(p)
    n_na = 700                               # n <= 17 500: the half-wave pair kernels serve every case
    X = _drop(rng, _columns(rng, p + n_na), n_na)
    assert np.all(np.sum(~np.isnan(X), axis=0) == p)
    _check_with_order(hip_ctx, X)


def test_three_tile_slots(hip_ctx):
    rng = np.random.default_rng(20000)
    n, p = 20000, 2 * TILE + 1 + 700
    X = _drop(rng, _columns(rng, n, 4), n - p)
    _check_with_order(hip_ctx, X)


@pytest.mark.parametrize("n_na", [0, 1, 9000 - 2, 9000 - 1, 9000])
def test_missingness_extremes(hip_ctx, n_na):
    rng = np.random.default_rng(n_na)
    n = 9000
    X = _drop(rng, _columns(rng, n, 4), n_na)
    _check_with_order(hip_ctx, X)


@pytest.mark.parametrize("form", ["nan_at_random_rows", "first_and_last_word"])
def test_scattered_missing_rows(hip_ctx, form):
    rng = np.random.default_rng(11)
    n = 9931                                 # the last bitset word holds 11 rows
    X = _columns(rng, n)
    if form == "nan_at_random_rows":
        X[rng.random(X.shape) < 0.12] = np.nan      # another count in every column
    else:
        X[:64:3, 0] = np.nan                 # the first word only
        X[n - 11:, 1] = np.nan               # the last word only, all of it
        X[0, 2] = X[n - 1, 2] = np.nan       # the first and the last row
        X[:64, 3] = np.nan                   # the first word, all of it
        X[rng.permutation(n)[:900], 4] = np.nan
        X[63:65, 4] = np.nan
        X[n - 12:n - 10, 4] = np.nan         # across the last word's edge
    _check_with_order(hip_ctx, X)


def test_finite_excluded_value_through_global_na(hip_ctx):
    """Rows excluded by a finite global_na value are kept out of the sort like NaN rows: the matrix entry on the raw data
    gives bit for bit what it gives on the same data with those cells already NaN, and that data passes the pair entry's
    check against the oracle."""
    rng = np.random.default_rng(13)
    n, S = 9800, 4
    X = _columns(rng, n, S)
    X[rng.random(X.shape) < 0.05] = np.nan
    gone = rng.random(X.shape) < 0.07
    X[gone] = 7.0                            # (a 7.0 the rounded columns hold already is excluded with them)
    Xn = np.where(X == 7.0, np.nan, X)
    assert 8192 < np.min(np.sum(~np.isnan(Xn), axis=0)) and np.max(np.sum(~np.isnan(Xn), axis=0)) < 8192 + 1024
    a, keep_a, rc_a = hip_ctx.matrix(np.asfortranarray(X), global_na=[np.nan, 7.0], scale_max=False)
    b, keep_b, rc_b = hip_ctx.matrix(np.asfortranarray(Xn), global_na=[np.nan], scale_max=False)
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(keep_a, keep_b) and np.array_equal(rc_a, rc_b)
    out, _cnt, _rsn = _check_with_order(hip_ctx, Xn)
    pi, pj = np.triu_indices(S, k=1)
    d = np.nanmax(np.abs(np.stack([a[1][pi, pj], a[2][pi, pj], a[3][pi, pj]], axis=1) - out[:, :3]))
    assert d <= ATOL, d


def test_ties_straddle_the_tile_boundary(hip_ctx):
    """Equal values at dense indices 8 190 .. 8 195 (two in the full tile, four in the sub-tile): below, inside and above
    the other values, and as the column's minimum beside the fill group."""
    rng = np.random.default_rng(17)
    n, n_na = 9900, 900
    X = _columns(rng, n)
    rows = rng.permutation(n)[:n_na]
    X[rows, :] = np.nan                      # the same rows in every column: one dense numbering
    present = np.flatnonzero(~np.isnan(X[:, 0]))
    at = present[TILE - 2:TILE + 4]
    for c, v in enumerate([0.123, 1.0, -100.0, 100.0, 0.0]):
        X[at, c] = v
    _check_with_order(hip_ctx, X)


def test_low_bits_fallback_at_a_tile_edge(hip_ctx):
    """The data of test_values_that_differ_only_in_their_low_bits, 10 % of the rows missing, p = 8 193: the columns whose
    one-word sort shows an inversion are sorted again whole, with three-word elements."""
    p, n_na = TILE + 1, 910
    n = p + n_na
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, 6))
    ulp = 2.0 ** -52
    k = rng.permutation(n) % 60000
    X[:, 0] = 1.0 + k * ulp
    X[:, 1] = -(3.0 + (rng.integers(0, 5000, n) * 4) * ulp)
    X[:, 2] = np.where(rng.random(n) < 0.5, X[:, 2], 7.0 + rng.integers(0, 3, n) * ulp * 8)
    X[:, 3] = np.round(X[:, 3], 2) + rng.integers(0, 2, n) * 2.0 ** -45
    X[:, 4] = np.where(rng.random(n) < 0.3, 0.0, rng.integers(-2, 3, n) * 2.0 ** -1070)
    X[::97, 4] = -0.0
    for c in range(6):
        X[rng.permutation(n)[:n_na], c] = np.nan
    for persp in ("global", "local"):
        _check(hip_ctx, X, perspective=persp)
    _check_with_order(hip_ctx, X)


def test_exchanged_state_is_unchanged(hip_ctx):
    """The one-rank sharded path: the pre-pass over a column range, then rec / hirow / tgroups rebuilt from order and the
    bitsets (what ranks exchange) equal what the pre-pass wrote itself, and the pairs equal the pair entry's."""
    import torch
    rng = np.random.default_rng(19)
    n, S, n_na = 9000 + 808, 6, 808
    X = np.asfortranarray(_drop(rng, _columns(rng, n, S), n_na))
    full = _check(hip_ctx, X, perspective="global")
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    hip_ctx.prepare_cols_dev(dX.data_ptr(), n, S, n, 0, S, S)
    hip_ctx.sync()
    arrays = hip_ctx.prep_arrays()

    def view(i, cols):
        ptr, bpc = arrays[i]

        class _D:
            __cuda_array_interface__ = {"shape": (bpc * cols,), "typestr": "|u1", "data": (ptr, False), "version": 2}
        return torch.as_tensor(_D(), device="cuda")

    derived = {i: view(i, S) for i in (1, 2, 4)}
    want = {i: t.clone() for i, t in derived.items()}
    for t in derived.values():
        t.fill_(0xEE)
    torch.cuda.synchronize()                       # (the fill runs on torch's stream, the rebuild on the context's)
    hip_ctx.expand_cols_dev(0, S)
    hip_ctx.sync()
    ntg = view(3, S).cpu().numpy().view(np.uint32).reshape(S, -1)[:, -16 + 7]
    n_pad = arrays[2][1] // 2
    for i, dt in ((1, np.uint32), (2, np.uint16)):
        w = want[i].cpu().numpy().view(dt).reshape(-1, n_pad, 2)
        g = derived[i].cpu().numpy().view(dt).reshape(-1, n_pad, 2)
        for c in range(S):
            assert np.array_equal(g[c >> 1, :n, c & 1], w[c >> 1, :n, c & 1]), (i, c)
    tg_w = want[4].cpu().numpy().view(np.uint32).reshape(S, -1)
    tg_g = derived[4].cpu().numpy().view(np.uint32).reshape(S, -1)
    for c in range(S):
        assert np.array_equal(tg_g[c, :ntg[c]], tg_w[c, :ntg[c]]), c
    P = S * (S - 1) // 2
    hip_ctx.set_pairs_combn(S, 0, P)
    out = torch.empty((P, 4), dtype=torch.float64, device="cuda")
    hip_ctx.run_dev(1, 0, False, 0, out.data_ptr())
    hip_ctx.sync()
    assert np.array_equal(out.cpu().numpy(), full[0], equal_nan=True)
