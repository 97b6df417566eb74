"""Input matrices whose ICI-Kendall-tau is known in closed form from integers, and the answers of the five selection
entries (topk, edges, class_medians, class_matrix, quantiles) on them.  Plain numpy: no GPU, no oracle, no S x S matrix
from the library.  Used by tests/test_designed_tau_host.py (against the CPU oracle and the brute-force checkers) and by
tests/test_gpu_designed_tau.py (against the kernels).

n rows, m = n (n - 1) / 2 pairs of rows, the base column 1, 2, ..., n (not from 0: the default global_na takes 0 as
missing).  Two families of complete columns without ties:
  swaps      column a = the base with its first k_a disjoint adjacent pairs exchanged, 0 <= k_a <= n // 2.
             Discordant row pairs between a and b: D = |k_a - k_b|.
  reversals  column a = the base with its first L_a entries reversed, 0 <= L_a <= n.
             D = |C(L_a, 2) - C(L_b, 2)|.
Every column is multiplied by a sign s_a = +-1.  Then
  num[a, b] = s_a s_b (m - 2 D)   (an integer),   raw[a, b] = num[a, b] / m   (one float64 division),
taumax = 1 for every pair, so cor == raw bit for bit and max_taumax == 1.0.  An all-NaN column is NA with every partner
(reason 1, all missing), a constant column with every other partner (reason 3, a single unique value); the other pairs
are untouched by them.

All ordering and counting is done on the integers num, where ties are exact; a float appears only as num / m, or as
R's mean() / quantile(type = 7) of two such values (tests/medians_checker.r_mean2, tests/quantiles_checker.type7)."""
import math

import numpy as np

from tests.medians_checker import r_mean2
from tests.quantiles_checker import type7

NA_REAL_BITS = np.uint64(0x7FF00000000007A2)
VALID, ALL_MISSING, CONSTANT = 0, 1, 2        # a column's kind
_FAR = np.int32(2 ** 30)                       # above every num: a partner that is no value sorts behind the others


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def na_filled(shape):
    a = np.empty(shape, dtype=np.float64)
    a.view(np.uint64)[...] = NA_REAL_BITS
    return a


class Design:
    """X [n, S] F-ordered float64; kind [S]; sign [S] (+-1, 0 for an NA column); disc [S]: k_a or C(L_a, 2);
    m; num [S, S] int32 (0 where the pair is NA or on the diagonal); valid [S, S] bool: a != b and neither is an NA
    column; raw [S, S] float64: num / m, NaN where not valid."""

    def __init__(self, family, X, kind, sign, disc, param):
        self.family, self.X, self.kind, self.sign, self.disc, self.param = family, X, kind, sign, disc, param
        self.n, self.S = X.shape
        self.m = self.n * (self.n - 1) // 2
        d, s = disc.astype(np.int32), sign.astype(np.int32)           # (every operand stays below 2^11)
        num = (np.int32(self.m) - 2 * np.abs(d[:, None] - d[None, :])) * s[:, None] * s[None, :]
        ok = kind == VALID
        self.valid = ok[:, None] & ok[None, :]
        np.fill_diagonal(self.valid, False)
        self.num = np.where(self.valid, num, np.int32(0))
        self._raw = None

    @property
    def raw(self):
        if self._raw is None:
            self._raw = np.where(self.valid, self.num / float(self.m), np.nan)
        return self._raw

    def value(self, num):
        """the float64 raw (== cor) of integer numerators"""
        return np.asarray(num, dtype=np.float64) / float(self.m)

    def reasons(self):
        """[S, S] int32 reason code per pair: 1 with an all-NaN column, else 3 with a constant one, else 0"""
        am, co = self.kind == ALL_MISSING, self.kind == CONSTANT
        r = np.zeros((self.S, self.S), dtype=np.int32)
        r[co[:, None] | co[None, :]] = 3
        r[am[:, None] | am[None, :]] = 1
        return r

    def reason_counts(self):
        iu, ju = np.triu_indices(self.S, k=1)
        return np.bincount(self.reasons()[iu, ju], minlength=5).astype(np.int64)

    def max_taumax(self):
        return 1.0 if self.valid.any() else -np.inf


def _assemble(family, n, S, seed, cols, disc_of, params, signs, n_all_missing, n_constant):
    """cols(param) -> the column of a parameter; the NA columns go to seeded positions among the S columns"""
    rng = np.random.default_rng(seed)
    n_na = n_all_missing + n_constant
    assert 0 <= n_na <= S
    kind = np.zeros(S, dtype=np.int32)
    where = rng.choice(S, size=n_na, replace=False)
    kind[where[:n_all_missing]] = ALL_MISSING
    kind[where[n_all_missing:]] = CONSTANT
    X = np.empty((n, S), order="F")
    sign = np.zeros(S, dtype=np.int32)
    disc = np.zeros(S, dtype=np.int64)
    param = np.full(S, -1, dtype=np.int64)
    good = np.nonzero(kind == VALID)[0]
    assert len(params) == len(signs) == len(good)
    for c, p, s in zip(good, params, signs):
        X[:, c] = s * cols(int(p))
        sign[c], disc[c], param[c] = s, disc_of(int(p)), p
    X[:, kind == ALL_MISSING] = np.nan
    X[:, kind == CONSTANT] = 2.5
    return Design(family, X, kind, sign, disc, param)


def _choices(rng, n_cols, values, params, signs, flip):
    if params is None:
        params = rng.choice(np.asarray(values), size=n_cols)
    if signs is None:
        signs = np.where(rng.random(n_cols) < flip, -1, 1)
    return np.asarray(params, dtype=np.int64), np.asarray(signs, dtype=np.int32)


def swaps(S, n, seed=0, params=None, signs=None, values=None, flip=0.5, n_all_missing=0, n_constant=0):
    """S columns of n rows; k_a drawn (seeded) from `values` (default 0 .. n // 2), or given as `params`; the signs
    drawn with P(-1) = flip, or given as `signs` (both per valid column, in column order)"""
    base = np.arange(1, n + 1, dtype=np.float64)

    def col(k):
        assert 0 <= k <= n // 2
        x = base.copy()
        x[0:2 * k:2], x[1:2 * k:2] = base[1:2 * k:2], base[0:2 * k:2]
        return x

    rng = np.random.default_rng(seed + 7919)
    p, s = _choices(rng, S - n_all_missing - n_constant, range(n // 2 + 1) if values is None else values, params, signs, flip)
    return _assemble("swaps", n, S, seed, col, lambda k: k, p, s, n_all_missing, n_constant)


def reversals(S, n, seed=0, params=None, signs=None, values=None, flip=0.5, n_all_missing=0, n_constant=0):
    """S columns of n rows; L_a drawn (seeded) from `values` (default 0 .. n), or given as `params`; signs as in swaps"""
    base = np.arange(1, n + 1, dtype=np.float64)

    def col(L):
        assert 0 <= L <= n
        x = base.copy()
        x[:L] = base[:L][::-1]
        return x

    rng = np.random.default_rng(seed + 7919)
    p, s = _choices(rng, S - n_all_missing - n_constant, range(n + 1) if values is None else values, params, signs, flip)
    return _assemble("reversals", n, S, seed, col, lambda L: L * (L - 1) // 2, p, s, n_all_missing, n_constant)


# ---- top-k -----------------------------------------------------------------------------------------------------------

def topk(d, k):
    """(idx [S, k] int32, -1 padded; num [S, k] int32 of the chosen; raw [S, k], NA_real_ padded; n_valid [S]): per
    sample the k valid partners of largest num, ties by the smaller partner index"""
    S = d.S
    key = np.where(d.valid, -d.num.astype(np.int64), np.int64(_FAR))
    order = np.argsort(key, axis=1, kind="stable")[:, :k]            # stable: equal num keep index order
    kk = order.shape[1]
    have = np.minimum(d.valid.sum(axis=1), k).astype(np.int32)
    take = np.arange(kk)[None, :] < have[:, None]
    idx = np.full((S, k), -1, dtype=np.int32)
    nums = np.zeros((S, k), dtype=np.int32)
    raw = na_filled((S, k))
    rows = np.arange(S)[:, None]
    idx[:, :kk] = np.where(take, order, -1)
    nums[:, :kk] = np.where(take, d.num[rows, order], 0)
    raw[:, :kk][take] = d.value(d.num[rows, order][take])
    return idx, nums, raw, have


# ---- edges -----------------------------------------------------------------------------------------------------------

def edges(d, min_num, absolute=False):
    """(ei, ej int32 in combn order; num [n_edges] int32; raw [n_edges]; n_edges; degree [S] int64): the valid pairs
    with num >= min_num (|num| with absolute).  raw >= min_num / m is the same rule: x -> x / m is strictly monotone on
    integers this small."""
    val = np.abs(d.num) if absolute else d.num
    ok = d.valid & (val >= min_num)
    degree = ok.sum(axis=1).astype(np.int64)
    ei, ej = np.nonzero(np.triu(ok, 1))                               # row-major upper triangle == combn order
    nums = d.num[ei, ej]
    return ei.astype(np.int32), ej.astype(np.int32), nums, d.value(nums), int(ei.shape[0]), degree


# ---- class medians / class matrix ------------------------------------------------------------------------------------

def _median_float(d, lo, hi, v):
    """R's median from the two middle numerators: lo / m for an odd count, else mean() of lo / m and hi / m"""
    out = na_filled(lo.shape)
    a, b = d.value(lo), d.value(hi)
    flat_o, flat_a, flat_b, flat_v = out.reshape(-1), a.reshape(-1), b.reshape(-1), v.reshape(-1)
    odd = (flat_v & 1) == 1
    flat_o[odd] = flat_a[odd] + 0.0
    for q in np.nonzero(~odd & (flat_v > 0))[0]:
        flat_o[q] = r_mean2(float(flat_a[q]) + 0.0, float(flat_b[q]) + 0.0)
    return out


def class_matrix(d, cls=None, n_class=1):
    """dict of [S, n_class] arrays for the cells (s, c): n_valid; lo, hi: the numerators of ranks (v - 1) >> 1 and
    v >> 1 among the cell's valid partners ascending; k_in: the rank of lo inside its run of equal numerators; run: that
    run's length; med: the median as float64 (== med_raw == med_cor), NA_real_ where n_valid == 0"""
    S = d.S
    cls = np.zeros(S, dtype=np.int64) if cls is None else np.asarray(cls)
    out = {k: np.zeros((S, n_class), dtype=np.int32) for k in ("n_valid", "lo", "hi", "k_in", "run")}
    for c in range(n_class):
        mem = np.nonzero(cls == c)[0]
        if mem.size == 0:
            continue
        sub = np.where(d.valid[:, mem], d.num[:, mem], _FAR)
        v = d.valid[:, mem].sum(axis=1).astype(np.int32)
        sub.sort(axis=1)
        rows = np.arange(S)
        have = v > 0
        lo = np.where(have, sub[rows, np.maximum(v - 1, 0) >> 1], 0)
        hi = np.where(have, sub[rows, np.minimum(v >> 1, mem.size - 1)], 0)
        start = (sub < lo[:, None]).sum(axis=1)
        out["n_valid"][:, c] = v
        out["lo"][:, c], out["hi"][:, c] = lo, hi
        out["k_in"][:, c] = np.where(have, (np.maximum(v - 1, 0) >> 1) - start, 0)
        out["run"][:, c] = np.where(have, (sub == lo[:, None]).sum(axis=1), 0)
    out["med"] = _median_float(d, out["lo"], out["hi"], out["n_valid"])
    return out


def class_medians(d, cls=None):
    """class_matrix's cell (s, cls[s]) per sample: dict of [S] arrays"""
    cls = np.zeros(d.S, dtype=np.int64) if cls is None else np.asarray(cls)
    full = class_matrix(d, cls, int(cls.max()) + 1)
    return {k: a[np.arange(d.S), cls] for k, a in full.items()}


# ---- quantiles and histogram -----------------------------------------------------------------------------------------

def group_counts(d, cls=None):
    """(cnt [G, 2 m + 1] int64: the pairs i < j of a group per numerator, cnt[g, num + m]; n_valid [G]; n_na [G]);
    G = 1 (all pairs) or, with cls, 3 (all, within-class, between-class)"""
    S, m = d.S, d.m
    off = ~np.eye(S, dtype=bool)
    masks = [off]
    if cls is not None:
        cls = np.asarray(cls)
        same = cls[:, None] == cls[None, :]
        masks = [off, off & same, off & ~same]
    G = len(masks)
    cnt = np.zeros((G, 2 * m + 1), dtype=np.int64)
    n_valid, n_na = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    for g, mask in enumerate(masks):
        ok = mask & d.valid
        both = np.bincount(d.num[ok].astype(np.int64) + m, minlength=2 * m + 1)     # every pair twice: (a, b), (b, a)
        assert np.all(both % 2 == 0)
        cnt[g] = both // 2
        n_valid[g] = int(ok.sum()) // 2
        n_na[g] = int(mask.sum()) // 2 - n_valid[g]
    return cnt, n_valid, n_na


def quantiles(d, probs, cls=None, counts=None):
    """(q [G, n_probs]: the type-7 quantile (== quantile_raw == quantile_cor); order2 [G, n_probs, 2]; ord_num
    [G, n_probs, 2] int64: the numerators of the two order statistics; n_valid, n_na [G])"""
    cnt, n_valid, n_na = group_counts(d, cls) if counts is None else counts
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    G = cnt.shape[0]
    q, order2 = na_filled((G, probs.shape[0])), na_filled((G, probs.shape[0], 2))
    ord_num = np.zeros((G, probs.shape[0], 2), dtype=np.int64)
    for g in range(G):
        v = int(n_valid[g])
        if v == 0:
            continue
        cum = np.cumsum(cnt[g])
        for k, p in enumerate(probs):
            index = 1.0 + float(v - 1) * float(p)
            lo, hi = int(math.floor(index)), int(math.ceil(index))
            na_, nb_ = (int(np.searchsorted(cum, r - 1, side="right")) - d.m for r in (lo, hi))   # rank r, 1-based
            a, b = float(d.value(na_)) + 0.0, float(d.value(nb_)) + 0.0
            ord_num[g, k] = na_, nb_
            order2[g, k] = a, b
            q[g, k] = type7(a, b, index, float(lo))
    return q, order2, ord_num, n_valid, n_na


def histogram(d, break_nums, cls=None, counts=None):
    """(hist [G, n_bins] int64; outside [G, 2]) for the breaks break_nums / m (strictly increasing integers): bin k
    holds break_nums[k] <= num < break_nums[k + 1], the last bin its right edge too"""
    cnt, _n_valid, _n_na = group_counts(d, cls) if counts is None else counts
    bn = np.asarray(break_nums, dtype=np.int64)
    assert bn.ndim == 1 and bn.shape[0] >= 2 and np.all(np.diff(bn) > 0)
    nums = np.arange(-d.m, d.m + 1)
    slot = np.searchsorted(bn, nums, side="right")            # 0 below, 1 + k in bin k, len(bn) at or above the last break
    slot[nums == bn[-1]] = len(bn) - 1
    G = cnt.shape[0]
    hist, outside = np.zeros((G, len(bn) - 1), dtype=np.int64), np.zeros((G, 2), dtype=np.int64)
    for g in range(G):
        per = np.zeros(len(bn) + 1, dtype=np.int64)
        np.add.at(per, slot, cnt[g])
        outside[g] = per[0], per[len(bn)]
        hist[g] = per[1:len(bn)]
    return hist, outside
