"""Input matrices whose ICI-Kendall-tau is known in closed form from integers, and the answers of the five selection
entries (topk, edges, class_medians, class_matrix, quantiles) on them, and of the eight later ones (anosim, permanova,
permdisp's table, padjust's sorted p-values, mst on +-base columns, the rectangle of cross with its top-k and class
table; hclust's reference is tests/hclust_checker.brute_hclust on Design.raw).  Plain numpy and Python ints: no GPU, no oracle, no S x S
matrix from the library.  Used by tests/test_designed_tau_host.py (against the CPU oracle and the brute-force checkers)
and by tests/test_gpu_designed_tau.py and tests/test_gpu_designed_tau_entries.py (against the kernels).

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

A third family, `censored` (class Censored, which has the formulas): tied, left-censored columns, on which taumax,
completeness and max_taumax differ from 1 and from each other, cor from raw, and "local" from "global".  There
raw = num / den and taumax = plus / den with a den that varies per pair under "local".

All ordering and counting is done on integers, where ties are exact: Design.key, which is num itself on swaps and
reversals and the exact dense rank of |num| / den, signed, on the censored family; Design.value(key) is the float64
raw.  A float appears only as that one division, as one more division by an entry's max_taumax (cor), or as R's mean()
/ quantile(type = 7) of two such values (tests/medians_checker.r_mean2, tests/quantiles_checker.type7)."""
import dataclasses
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
        self.family, self.sign, self.disc, self.param = family, sign, disc, param
        self._set_columns(X, kind)
        d, s = disc.astype(np.int32), sign.astype(np.int32)           # (every operand stays below 2^11)
        num = (np.int32(self.m) - 2 * np.abs(d[:, None] - d[None, :])) * s[:, None] * s[None, :]
        self.num = np.where(self.valid, num, np.int32(0))

    def _set_columns(self, X, kind):
        """what every family shares: X, kind, n, S, m, valid, and the caches of raw and of the triangle"""
        self.X, self.kind = X, kind
        self.n, self.S = X.shape
        self.m = self.n * (self.n - 1) // 2
        ok = kind == VALID
        self.valid = ok[:, None] & ok[None, :]
        np.fill_diagonal(self.valid, False)
        self._raw = self._tri = None
        return ok

    def columns(self, which):
        """the design of the columns `which` alone"""
        return Design(self.family, np.asfortranarray(self.X[:, which]), self.kind[which], self.sign[which], self.disc[which],
                      self.param[which])

    @property
    def key(self):
        """[S, S] int32, the integers that order raw exactly, in -K .. K with key(-raw) == -key(raw): here num itself"""
        return self.num

    @property
    def K(self):
        return self.m

    @property
    def raw(self):
        if self._raw is None:
            self._raw = np.where(self.valid, self.num / float(self.m), np.nan)
        return self._raw

    def value(self, key):
        """the float64 raw of integer keys (here the numerators: num / m)"""
        return np.asarray(key, dtype=np.float64) / float(self.m)

    def under(self, perspective):
        """the design as a perspective sees it: complete columns look the same under both"""
        return self

    def taumax(self, a, b):
        return np.ones(np.broadcast(a, b).shape)

    def completeness(self, a, b):
        return np.ones(np.broadcast(a, b).shape)

    def pvalue_id(self, a, b, one_sided=False):
        """an integer per pair that the p-value is a function of: num (|num| two-sided); n and the ties are constant"""
        v = self.num[a, b].astype(np.int64)
        return v if one_sided else np.abs(v)

    def planes(self, mask=None, scale_max=True, pvalue=None):
        """[5, S, S]: cor, raw, pvalue, taumax, completeness as the library's matrices have them, NaN where the pair is
        not valid and on the diagonal.  cor is raw / max_taumax(mask) under scale_max; pvalue: an [S, S] plane from
        outside (it has no closed form), else NaN."""
        out = np.full((5, self.S, self.S), np.nan)
        a, b = np.nonzero(self.valid)
        out[1] = self.raw
        out[0][a, b] = cor_value(self.raw[a, b], self.max_taumax(mask), scale_max)
        if pvalue is not None:
            out[2][a, b] = pvalue[a, b]
        out[3][a, b], out[4][a, b] = self.taumax(a, b), self.completeness(a, b)
        return out

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

    def max_taumax(self, mask=None):
        """the largest taumax of the valid pairs (of those in `mask` [S, S]); -inf when there is none"""
        return 1.0 if (self.valid if mask is None else self.valid & mask).any() else -np.inf


def cor_value(raw, mx, scale_max=True):
    """cor of a float64 raw: one more float64 division by the entry's max_taumax, or raw itself"""
    return np.asarray(raw, dtype=np.float64) / mx if scale_max else np.asarray(raw, dtype=np.float64)


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


# ---- the third family: tied, left-censored columns -------------------------------------------------------------------

COUNT_FIELDS = ("n", "missing", "dis", "ntie", "xtie", "ytie", "x0", "x1", "y0", "y1", "tot")
_BOTTOM = {}


def _sgn(v):
    return (v > 0) - (v < 0)


def _bottom_tables(lib, B0):
    """(cmd, cpd [2, L, L]; J, U [L, L]) over pairs of library subsets, by a plain count over the row pairs of the
    bottom block: concordant minus discordant, concordant plus discordant (the row pairs tied in neither column), the
    size of the intersection and of the union.  Index 0: every row kept; 1: the rows of the intersection dropped (what
    the local perspective does to rows missing in both columns).  A row of the subset holds 0, below every base value."""
    if (lib, B0) not in _BOTTOM:
        L = len(lib)
        cmd, cpd = np.zeros((2, L, L), dtype=np.int32), np.zeros((2, L, L), dtype=np.int32)
        J, U = np.zeros((L, L), dtype=np.int32), np.zeros((L, L), dtype=np.int32)
        filled = [[0 if r in set(A) else r + 1 for r in range(B0)] for A in lib]
        for p, A in enumerate(lib):
            for q, B in enumerate(lib):
                both = set(A) & set(B)
                J[p, q], U[p, q] = len(both), len(set(A) | set(B))
                for drop in (0, 1):
                    rows = [r for r in range(B0) if not (drop and r in both)]
                    va, vb = [filled[p][r] for r in rows], [filled[q][r] for r in rows]
                    for x in range(len(rows)):
                        for y in range(x + 1, len(rows)):
                            s = _sgn(va[x] - va[y]) * _sgn(vb[x] - vb[y])
                            cmd[drop, p, q] += s
                            cpd[drop, p, q] += abs(s)
        _BOTTOM[(lib, B0)] = cmd, cpd, J, U
    return _BOTTOM[(lib, B0)]


@dataclasses.dataclass
class _Columns:
    """what the views of one censored design share: the shape, the libraries, and how each column was made"""
    n: int
    B0: int
    c: int
    t: int
    h: int
    variant: str
    lib: tuple           # the c-subsets of the bottom block
    states: np.ndarray   # [n_states, h] int8
    X: np.ndarray
    kind: np.ndarray
    sign: np.ndarray
    st: np.ndarray       # per column: its state's index, its subset's index
    lb: np.ndarray


class Censored(Design):
    """A design of tied, left-censored columns as ONE perspective sees it (under(perspective) gives the other).
    n = B0 + 2 h rows.  Rows 0 .. B0 - 1 are the bottom block, base values 1 .. B0; the c rows of the column's library
    subset M_a are NaN there (variant "nan") or 0.5 (variant "ties": the same integers, nothing missing).  Rows
    B0 + 2 p, B0 + 2 p + 1 are the adjacent pair p of the upper part, base values B0 + 2 p + 1 and + 2: in order
    (state +1), exchanged (-1) or both the lower value (0, exactly t of the h); a column sign -1 reflects the upper part
    alone, v -> B0 + n + 1 - v.  The reference's fill (min - 0.1) keeps the NaN rows one tie group below everything.

    For a pair (a, b): j = |M_a & M_b|, u = |M_a | M_b|, drop = j under "local" on NaN columns and 0 otherwise,
    n_eff = n - drop, tot = C(n_eff, 2), c' = c - drop, xtie = ytie = t + C(c', 2), den = tot - xtie (so
    sqrt((tot - xtie)(tot - ytie)) == den exactly),
      num  = (B0 - drop) 2 h + cmd(M_a, M_b, drop) + sign_a sign_b (C(2 h, 2) - h + s_a . s_b)
      plus = (B0 - drop) 2 h + cpd(M_a, M_b, drop) +               (C(2 h, 2) - h + |s_a| . |s_b|)
    raw = num / den, taumax = plus / den (one float64 division each), completeness = 1 - (u - drop) / n_eff, and the
    eleven counts follow (counts()).  All of it is a function of the two columns' (state, subset, sign), so the integers
    are kept as tables over the distinct such types.

    key [S, S] int32: the dense rank of |num| / den among the design's distinct fractions (compared as fractions), with
    the sign of num, 0 for num == 0; K the largest; value(key) the float64 num / den.  den varies under "local", so
    num alone does not order raw there."""

    def __init__(self, cols, perspective):
        from fractions import Fraction
        assert perspective in ("global", "local")
        c = self.cols = cols
        self.family, self.perspective, self.sign = "censored", perspective, c.sign
        self.disc = self.param = None                                     # (the other families' parameters)
        self._views = {perspective: self}
        ok = self._set_columns(c.X, c.kind)
        n, B0, cc, t, h = c.n, c.B0, c.c, c.t, c.h
        local = perspective == "local" and c.variant == "nan"
        trip = np.stack([c.st, c.lb, c.sign.astype(np.int64)], axis=1)[ok]
        if len(trip):
            types, ty = np.unique(trip, axis=0, return_inverse=True)
        else:
            types, ty = np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.int64)
        T = len(types)
        St = c.states[types[:, 0]].astype(np.int32)                       # [T, h]
        sg = types[:, 2].astype(np.int32)
        la = types[:, 1]
        cmd, cpd, J, U = _bottom_tables(c.lib, B0)
        take = lambda a: a[la][:, la]                                     # noqa: E731
        self._j, self._u = take(J).astype(np.int8), take(U).astype(np.int8)
        self._drop = self._j.copy() if local else np.zeros((T, T), dtype=np.int8)
        self._adot = (np.abs(St) @ np.abs(St).T).astype(np.int8)
        drop = self._drop.astype(np.int32)
        upper = h * (2 * h - 1) - h
        both = (B0 - drop) * (2 * h)
        self._num = both + take(cmd[1 if local else 0]) + (sg[:, None] * sg[None, :]) * (np.int32(upper) + St @ St.T)
        self._plus = both + take(cpd[1 if local else 0]) + np.int32(upper) + self._adot
        # what depends on drop alone
        dr = np.arange(cc + 1, dtype=np.int64)
        self.by_drop = {"n_eff": n - dr, "tot": (n - dr) * (n - dr - 1) // 2, "c1": cc - dr}
        self.by_drop["xtie"] = t + self.by_drop["c1"] * (self.by_drop["c1"] - 1) // 2
        self.by_drop["den"] = self.by_drop["tot"] - self.by_drop["xtie"]
        assert self.by_drop["den"].min() > 0
        # the key: fractions |num| / den ranked exactly, over the codes |num| (c + 1) + drop that occur
        code = np.abs(self._num).astype(np.int64) * (cc + 1) + drop
        present = np.nonzero(np.bincount(code.ravel(), minlength=1))[0]
        fraction_of = {int(v): Fraction(int(v) // (cc + 1), int(self.by_drop["den"][int(v) % (cc + 1)])) for v in present}
        fr = sorted(set(fraction_of.values()) | {Fraction(0)})
        rank_of = {f: r for r, f in enumerate(fr)}                        # Fraction(0) has rank 0
        self._K = len(fr) - 1
        lut = np.zeros(int(code.max(initial=0)) + 1, dtype=np.int32)
        for v in present:
            lut[v] = rank_of[fraction_of[int(v)]]
        self._key = lut[code] * np.sign(self._num).astype(np.int32)
        pos = np.array([float(f.numerator) / float(f.denominator) for f in fr])    # equal fractions: equal quotients
        self.values = np.concatenate([-pos[:0:-1], pos])                  # index K + key
        self.distinct_doubles = bool(np.all(np.diff(self.values) > 0))
        # per sample: its type, T for an NA column -- a padded row and column of the tables
        self.ty = np.full(self.S, T, dtype=np.int64)
        self.ty[ok] = ty
        self.num = self._matrix(self._num)
        self._keym = self._matrix(self._key)

    def _matrix(self, table, dtype=np.int32):
        """[S, S] from a [T, T] table: 0 where the pair is not valid"""
        T = table.shape[0]
        pad = np.zeros((T + 1, T + 1), dtype=dtype)
        pad[:T, :T] = table
        out = pad[self.ty[:, None], self.ty[None, :]]
        out[~self.valid] = 0
        return out

    def _of(self, table, a, b):
        """the table's entries for pairs (a, b); for an NA column some entry: the caller masks those pairs"""
        last = table.shape[0] - 1
        return table[np.minimum(self.ty[a], last), np.minimum(self.ty[b], last)]

    key = property(lambda self: self._keym)
    K = property(lambda self: self._K)

    @property
    def raw(self):
        if self._raw is None:
            self._raw = np.where(self.valid, self.value(self._keym), np.nan)
        return self._raw

    def value(self, key):
        return self.values[np.asarray(key, dtype=np.int64) + self._K]

    def under(self, perspective):
        if perspective not in self._views:
            self._views[perspective] = Censored(self.cols, perspective)
            self._views[perspective]._views = self._views
        return self._views[perspective]

    def columns(self, which):
        """the design of the columns `which` alone, under the same perspective"""
        c = self.cols
        return Censored(dataclasses.replace(c, X=np.asfortranarray(c.X[:, which]), kind=c.kind[which], sign=c.sign[which],
                                            st=c.st[which], lb=c.lb[which]), self.perspective)

    # -- the integers of pairs (a, b): index arrays of valid pairs
    def plus(self, a, b):
        return self._of(self._plus, a, b).astype(np.int64)

    def drop(self, a, b):
        return self._of(self._drop, a, b).astype(np.int64)

    def den(self, a, b):
        return self.by_drop["den"][self.drop(a, b)]

    def n_eff(self, a, b):
        return self.by_drop["n_eff"][self.drop(a, b)]

    def missing(self, a, b):
        if self.cols.variant != "nan":
            return np.zeros(np.broadcast(a, b).shape, dtype=np.int64)
        return self._of(self._u, a, b).astype(np.int64) - self.drop(a, b)

    def taumax(self, a, b):
        return self.plus(a, b).astype(np.float64) / self.den(a, b).astype(np.float64)

    def completeness(self, a, b):
        """the float64 expression 1.0 - missing / n_eff"""
        return 1.0 - self.missing(a, b).astype(np.float64) / self.n_eff(a, b).astype(np.float64)

    def counts(self, a, b):
        """[P, 11] int64 in COUNT_FIELDS order"""
        c = self.cols
        dr = self.drop(a, b)
        j = self._of(self._j, a, b).astype(np.int64)
        num, plus = self.num[a, b].astype(np.int64), self.plus(a, b)
        c1, xt = self.by_drop["c1"][dr], self.by_drop["xtie"][dr]
        ntie = (j - dr) * (j - dr - 1) // 2 + self._of(self._adot, a, b).astype(np.int64) + 2 * c.t - c.h
        # tie groups: one of c' rows and t of two.  x0 is the reference's sum of g (g - 1)(g - 2) HALVED (it divides
        # t0 by two, kendallc.cpp's count_rank_tie); a group of two adds nothing to it and 2 * 1 * 9 to x1
        x0, x1 = c1 * (c1 - 1) * (c1 - 2) // 2, c1 * (c1 - 1) * (2 * c1 + 5) + 18 * c.t
        assert np.all((plus - num) % 2 == 0)
        return np.stack([self.by_drop["n_eff"][dr], self.missing(a, b), (plus - num) // 2, ntie, xt, xt, x0, x1, x0, x1,
                         self.by_drop["tot"][dr]], axis=-1)

    def pvalue_id(self, a, b, one_sided=False):
        """one integer per distinct (num, den, n_eff) -- (|num|, den, n_eff) two-sided: den and n_eff follow from drop"""
        v = self.num[a, b].astype(np.int64)
        return (v if one_sided else np.abs(v)) * (self.cols.c + 1) + self.drop(a, b)

    def max_taumax(self, mask=None, columns=None):
        """the exact maximum of the fractions plus / den over the valid pairs (of those in `mask`, or of those among
        the columns `columns`), as its float64"""
        from fractions import Fraction
        if mask is None:        # from the type table alone: a cell counts when both types occur (its own twice)
            T = self._plus.shape[0]
            ty = self.ty if columns is None else self.ty[np.asarray(columns)]
            cnt = np.bincount(ty[ty < T], minlength=T)
            there = (cnt[:, None] > 0) & (cnt[None, :] > 0)
            there[np.arange(T), np.arange(T)] = cnt >= 2
            best = None
            for dr in range(self.cols.c + 1):
                sel = there & (self._drop == dr)
                if sel.any():
                    f = Fraction(int(self._plus[sel].max()), int(self.by_drop["den"][dr]))
                    best = f if best is None or f > best else best
            return -np.inf if best is None else float(best.numerator) / float(best.denominator)
        ok = self.valid & mask
        a, b = np.nonzero(ok)
        if len(a) == 0:
            return -np.inf
        T1 = self._plus.shape[0] + 1
        cells = np.unique(self.ty[a] * T1 + self.ty[b])
        ta, tb = cells // T1, cells % T1
        pd = np.unique(np.stack([self._plus[ta, tb].astype(np.int64), self.by_drop["den"][self._drop[ta, tb]]], axis=1),
                       axis=0)
        best = max(Fraction(int(p), int(q)) for p, q in pd)
        return float(best.numerator) / float(best.denominator)


def censored(S, n, B0, c, t, seed=0, variant="nan", perspective="global", n_lib=20, n_states=None, distinct=True,
             own_state=False, twin=True, flip=0.5, n_all_missing=0, n_constant=0, max_overlap=None):
    """S columns of the censored family (class Censored).  The valid columns draw their (state, subset) from n_states
    seeded state vectors and n_lib seeded c-subsets of the bottom block: without replacement when `distinct` (no two
    columns alike), else with.  own_state: every column has a state of its own (no two columns tie the same pairs, so
    no taumax is 1 under either perspective, the twin's apart).  twin: the second valid column is then given the first
    one's (state, subset) -- the one pair of the design with taumax == 1, and it lies in the first block of the
    triangle.  signs with P(-1) = flip.  The NA columns go to seeded positions, as in the other families.  max_overlap: no two library subsets share more rows
    than that (then taumax == 1 under "local" needs identical subsets, as under "global")."""
    import itertools
    h = (n - B0) // 2
    assert n == B0 + 2 * h and n <= 200 and 0 <= t <= h and 0 < c < B0 and variant in ("nan", "ties")
    rng = np.random.default_rng(seed + 7919)
    subsets = list(itertools.combinations(range(B0), c))
    if max_overlap is None:
        lib = tuple(subsets[i] for i in sorted(rng.choice(len(subsets), size=min(n_lib, len(subsets)), replace=False)))
    else:   # no two subsets share more than max_overlap rows: with c - max_overlap >= 2 a NaN tie group survives "local"
        lib = []
        for i in rng.permutation(len(subsets)):
            if len(lib) < n_lib and all(len(set(subsets[i]) & set(m)) <= max_overlap for m in lib):
                lib.append(subsets[i])
        assert len(lib) == n_lib
        lib = tuple(sorted(lib))
    n_cols = S - n_all_missing - n_constant
    if n_states is None:
        n_states = n_cols if own_state else -(-n_cols // len(lib)) + 1
    assert math.comb(h, t) >= n_states
    states, zero_sets = [], set()
    while len(states) < n_states:                                         # no two states tie the same t pairs
        s = rng.choice([-1, 1], size=h)
        zeros = tuple(sorted(rng.choice(h, size=t, replace=False).tolist()))
        if zeros in zero_sets:
            continue
        zero_sets.add(zeros)
        s[list(zeros)] = 0
        states.append(s)
    states = np.array(states, dtype=np.int8).reshape(n_states, h)
    n_combo = n_states * len(lib)
    assert not distinct or n_combo >= n_cols
    if own_state:
        assert n_states >= n_cols
        combo = np.arange(n_cols) * len(lib) + rng.choice(len(lib), size=n_cols)
    else:
        combo = rng.choice(n_combo, size=n_cols, replace=not distinct)
    if twin and n_cols > 1:
        combo[1] = combo[0]
    signs = np.where(rng.random(n_cols) < flip, -1, 1)
    if twin and n_cols > 1:
        signs[1] = signs[0]

    kind = np.zeros(S, dtype=np.int32)
    where = np.random.default_rng(seed).choice(S, size=n_all_missing + n_constant, replace=False)
    kind[where[:n_all_missing]] = ALL_MISSING
    kind[where[n_all_missing:]] = CONSTANT
    good = np.nonzero(kind == VALID)[0]
    X = np.empty((n, S), order="F")
    cols = _Columns(n, B0, c, t, h, variant, lib, states, X, kind, np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int64),
                    np.zeros(S, dtype=np.int64))
    X[:, kind == ALL_MISSING] = np.nan
    X[:, kind == CONSTANT] = 2.5
    low = B0 + 1 + 2 * np.arange(h, dtype=np.float64)                     # the lower base value of each adjacent pair
    for col, q, sg in zip(good, combo, signs):
        st, lb = int(q) // len(lib), int(q) % len(lib)
        s = states[st]
        x = np.arange(1, n + 1, dtype=np.float64)
        x[B0::2] = np.where(s == -1, low + 1, low)
        x[B0 + 1::2] = np.where(s == 1, low + 1, low)
        if sg < 0:
            x[B0:] = B0 + n + 1 - x[B0:]
        x[list(lib[lb])] = np.nan if variant == "nan" else 0.5
        X[:, col] = x
        cols.st[col], cols.lb[col], cols.sign[col] = st, lb, sg
    return Censored(cols, perspective)


def valid_columns(d):
    """the design's valid columns alone: no NA pair (PERMANOVA sums per class only then)"""
    return d.columns(np.nonzero(d.kind == VALID)[0])


def carried(d, a, b, mx, scale_max=True, pvalue=None):
    """[5, *a.shape]: cor, raw, pvalue, taumax, completeness that an entry carries for the pairs (a, b); where b < 0 (no
    partner) NA_real_.  mx: the entry's max_taumax, cor's divisor under scale_max; pvalue: an array like a from outside,
    else that plane is left NaN."""
    a, b = np.broadcast_arrays(np.asarray(a), np.asarray(b))
    out = na_filled((5,) + a.shape)
    sel = b >= 0
    aa, bb = a[sel], b[sel]
    raw = d.value(d.key[aa, bb])
    out[1][sel], out[0][sel] = raw, cor_value(raw, mx, scale_max)
    out[2][sel] = np.nan if pvalue is None else np.asarray(pvalue)[sel]
    out[3][sel], out[4][sel] = d.taumax(aa, bb), d.completeness(aa, bb)
    return out


# ---- top-k -----------------------------------------------------------------------------------------------------------

def _topk(d, num, valid, k):
    """topk over the rows of any [rows, partners] block of numerators"""
    S = num.shape[0]
    key = np.where(valid, -num.astype(np.int64), np.int64(_FAR))
    order = np.argsort(key, axis=1, kind="stable")[:, :k]            # stable: equal num keep index order
    kk = order.shape[1]
    have = np.minimum(valid.sum(axis=1), k).astype(np.int32)
    take = np.arange(kk)[None, :] < have[:, None]
    idx = np.full((S, k), -1, dtype=np.int32)
    nums = np.zeros((S, k), dtype=np.int32)
    raw = na_filled((S, k))
    rows = np.arange(S)[:, None]
    idx[:, :kk] = np.where(take, order, -1)
    nums[:, :kk] = np.where(take, num[rows, order], 0)
    raw[:, :kk][take] = d.value(num[rows, order][take])
    return idx, nums, raw, have


def topk(d, k):
    """(idx [S, k] int32, -1 padded; num [S, k] int32 of the chosen; raw [S, k], NA_real_ padded; n_valid [S]): per
    sample the k valid partners of largest num, ties by the smaller partner index"""
    return _topk(d, d.key, d.valid, k)


# ---- edges -----------------------------------------------------------------------------------------------------------

def edges(d, min_num, absolute=False, also=None):
    """(ei, ej int32 in combn order; num [n_edges] int32; raw [n_edges]; n_edges; degree [S] int64): the valid pairs
    with num >= min_num (|num| with absolute).  raw >= min_num / m is the same rule: x -> x / m is strictly monotone on
    integers this small.  On a design whose key is not num, min_num and the third item are keys.  also: a symmetric
    [S, S] bool mask that a pair must pass as well (a bound on completeness or on the p-value)."""
    val = np.abs(d.key) if absolute else d.key
    ok = d.valid & (val >= min_num)
    if also is not None:
        ok &= also
    degree = ok.sum(axis=1).astype(np.int64)
    ei, ej = np.nonzero(np.triu(ok, 1))                               # row-major upper triangle == combn order
    nums = d.key[ei, ej]
    return ei.astype(np.int32), ej.astype(np.int32), nums, d.value(nums), int(ei.shape[0]), degree


# ---- class medians / class matrix ------------------------------------------------------------------------------------

def median_cor(d, cells, mx):
    """med_cor of class_matrix's or class_medians' dict under scale_max: the median of raw / mx, mx the entry's
    max_taumax.  Division by a positive constant keeps the order, so the two middle values are those of raw."""
    return _median_float(d, cells["lo"], cells["hi"], cells["n_valid"], mx)


def _median_float(d, lo, hi, v, mx=None):
    """R's median from the two middle numerators: lo / m for an odd count, else mean() of lo / m and hi / m"""
    out = na_filled(lo.shape)
    a, b = d.value(lo), d.value(hi)
    if mx is not None:
        a, b = a / mx, b / mx
    flat_o, flat_a, flat_b, flat_v = out.reshape(-1), a.reshape(-1), b.reshape(-1), v.reshape(-1)
    odd = (flat_v & 1) == 1
    flat_o[odd] = flat_a[odd] + 0.0
    for q in np.nonzero(~odd & (flat_v > 0))[0]:
        flat_o[q] = r_mean2(float(flat_a[q]) + 0.0, float(flat_b[q]) + 0.0)
    return out


def _class_cells(d, num, valid, cls, n_class):
    """class_matrix over the rows of any [rows, partners] block of numerators; cls: a class per partner"""
    S = num.shape[0]
    cls = np.asarray(cls)
    out = {k: np.zeros((S, n_class), dtype=np.int32) for k in ("n_valid", "lo", "hi", "k_in", "run")}
    for c in range(n_class):
        mem = np.nonzero(cls == c)[0]
        if mem.size == 0:
            continue
        sub = np.where(valid[:, mem], num[:, mem], _FAR)
        v = valid[:, mem].sum(axis=1).astype(np.int32)
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


def class_matrix(d, cls=None, n_class=1):
    """dict of [S, n_class] arrays for the cells (s, c): n_valid; lo, hi: the numerators of ranks (v - 1) >> 1 and
    v >> 1 among the cell's valid partners ascending; k_in: the rank of lo inside its run of equal numerators; run: that
    run's length; med: the median as float64 (== med_raw == med_cor), NA_real_ where n_valid == 0"""
    cls = np.zeros(d.S, dtype=np.int64) if cls is None else np.asarray(cls)
    return _class_cells(d, d.key, d.valid, cls, n_class)


def class_medians(d, cls=None):
    """class_matrix's cell (s, cls[s]) per sample: dict of [S] arrays"""
    cls = np.zeros(d.S, dtype=np.int64) if cls is None else np.asarray(cls)
    full = class_matrix(d, cls, int(cls.max()) + 1)
    return {k: a[np.arange(d.S), cls] for k, a in full.items()}


# ---- quantiles and histogram -----------------------------------------------------------------------------------------

def group_counts(d, cls=None):
    """(cnt [G, 2 m + 1] int64: the pairs i < j of a group per numerator, cnt[g, num + m]; n_valid [G]; n_na [G]);
    G = 1 (all pairs) or, with cls, 3 (all, within-class, between-class)"""
    S, m = d.S, d.K
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
        both = np.bincount(d.key[ok].astype(np.int64) + m, minlength=2 * m + 1)     # every pair twice: (a, b), (b, a)
        assert np.all(both % 2 == 0)
        cnt[g] = both // 2
        n_valid[g] = int(ok.sum()) // 2
        n_na[g] = int(mask.sum()) // 2 - n_valid[g]
    return cnt, n_valid, n_na


def quantiles(d, probs, cls=None, counts=None, mx=None):
    """(q [G, n_probs]: the type-7 quantile (== quantile_raw == quantile_cor); order2 [G, n_probs, 2]; ord_num
    [G, n_probs, 2] int64: the numerators of the two order statistics; n_valid, n_na [G]).  mx: q is quantile_cor under
    scale_max, the type-7 quantile of the two order statistics each divided by mx (order2 stays raw)."""
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
            na_, nb_ = (int(np.searchsorted(cum, r - 1, side="right")) - d.K for r in (lo, hi))   # rank r, 1-based
            a, b = float(d.value(na_)) + 0.0, float(d.value(nb_)) + 0.0
            ord_num[g, k] = na_, nb_
            order2[g, k] = a, b
            q[g, k] = type7(a, b, index, float(lo)) if mx is None else type7(a / mx + 0.0, b / mx + 0.0, index, float(lo))
    return q, order2, ord_num, n_valid, n_na


def histogram(d, break_nums, cls=None, counts=None):
    """(hist [G, n_bins] int64; outside [G, 2]) for the breaks break_nums / m (strictly increasing integers): bin k
    holds break_nums[k] <= num < break_nums[k + 1], the last bin its right edge too"""
    cnt, _n_valid, _n_na = group_counts(d, cls) if counts is None else counts
    bn = np.asarray(break_nums, dtype=np.int64)
    assert bn.ndim == 1 and bn.shape[0] >= 2 and np.all(np.diff(bn) > 0)
    nums = np.arange(-d.K, d.K + 1)
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


# ---- the triangle as integers (anosim, permanova, padjust) -----------------------------------------------------------

def triangle(d):
    """(i, j int32, k int32) of the VALID pairs i < j in combn order, k = num + m in 0 .. 2 m; n_na: the other pairs of
    the triangle.  Kept on the design: every reference below starts from it."""
    if getattr(d, "_tri", None) is None:
        iu, ju = np.triu_indices(d.S, k=1)
        ok = d.valid[iu, ju]
        i, j = iu[ok].astype(np.int32), ju[ok].astype(np.int32)
        d._tri = (i, j, d.key[i, j] + np.int32(d.K), int(ok.shape[0] - i.shape[0]))
    return d._tri


def class_hist(d, lab, n_class):
    """[n_class, 2 m + 1] int64: the valid pairs i < j whose two samples both have class c under the labelling `lab`,
    per numerator (column num + m)"""
    i, j, k, _n_na = triangle(d)
    lab = np.asarray(lab, dtype=np.int64)
    width = 2 * d.K + 1
    li = lab[i]
    same = li == lab[j]
    return np.bincount(li[same] * width + k[same], minlength=n_class * width).reshape(n_class, width)


def _labellings(d, cls, labellings):
    cls = np.asarray(cls, dtype=np.int64)
    perms = np.asarray(labellings, dtype=np.int64).reshape(-1, d.S)
    return cls, perms, [cls] + list(perms)


def anosim(d, cls, n_class, labellings):
    """tests/anosim_checker.brute_anosim's dict (without r2, i, j) from the integers.  A value's doubled rank in
    descending num is 2 * above + cnt + 1, `above` the values of larger num and cnt those equal to it: the checker's
    below + upto + 1.  w2 and nw of a labelling are histogram . table and the histogram's sum."""
    from tests import anosim_checker as ac
    cls, perms, labs = _labellings(d, cls, labellings)
    _i, _j, k, n_na = triangle(d)
    M = int(k.shape[0])
    cnt = np.bincount(k, minlength=2 * d.K + 1).astype(np.int64)
    above = np.cumsum(cnt[::-1])[::-1] - cnt
    r2 = 2 * above + cnt + 1                                         # (at most 2 M < 2^26: the sums below stay in int64)
    assert M == 0 or int(np.dot(cnt, r2)) == M * (M + 1)
    w2, nw = np.zeros(len(labs), dtype=np.int64), np.zeros(len(labs), dtype=np.int64)
    for q, lab in enumerate(labs):
        h = class_hist(d, lab, n_class)
        if q == 0:
            class_w2, class_nw = h @ r2, h.sum(axis=1)
        w2[q], nw[q] = int(np.dot(h.sum(axis=0), r2)), int(h.sum())
    obs = ac.statistic(M, w2[0], nw[0])
    stats = [ac.statistic(M, a, b) for a, b in zip(w2[1:], nw[1:])]
    n_ge = 0 if obs is None else sum(1 for f in stats if f is not None and f >= obs)
    W2, nW = int(w2[0]), int(nw[0])
    F = ac.Fraction
    return {
        "n_pairs": np.array([M, n_na], dtype=np.int64), "w2": w2, "nw": nw, "n_ge": n_ge,
        "n_undefined": sum(1 for f in stats if f is None), "class_w2": class_w2, "class_nw": class_nw,
        "statistic": ac.to_double(obs),
        "pvalue": ac.na_real() if obs is None else float(F(1 + n_ge, 1 + len(stats))),
        "perm_statistic": np.array([ac.to_double(f) for f in stats], dtype=np.float64),
        "class_mean_rank": np.array([ac.to_double(F(int(a), 2 * int(b)) if b else None)
                                     for a, b in zip(class_w2, class_nw)], dtype=np.float64),
        "within_mean_rank": ac.to_double(F(W2, 2 * nW) if nW else None),
        "between_mean_rank": ac.to_double(F(M * (M + 1) - W2, 2 * (M - nW)) if M > nW else None),
    }


def q_table(d):
    """q per numerator, index num + m: tests/permanova_checker.quantise(num / m) in Python ints (dtype object)"""
    from tests.permanova_checker import quantise
    return np.array([quantise(float(d.value(v))) for v in range(-d.K, d.K + 1)], dtype=object)


def permanova(d, cls, n_class, labellings):
    """tests/permanova_checker.brute_permanova's dict (without "exact") from the integers: q is a function of num
    alone, so Q and every A_c are histogram . table in Python ints.  With an NA pair every A_c is 0."""
    from tests import permanova_checker as pc
    cls, perms, labs = _labellings(d, cls, labellings)
    _i, _j, k, n_na = triangle(d)
    table = q_table(d)
    cnt = np.bincount(k, minlength=2 * d.K + 1)
    used = np.nonzero(cnt)[0]
    Q = sum(int(cnt[v]) * table[v] for v in used)
    class_q, sizes = [], []
    for lab in labs:
        sizes.append([int(v) for v in np.bincount(lab, minlength=n_class)])
        if n_na:
            class_q.append([0] * n_class)
            continue
        h = class_hist(d, lab, n_class)[:, used].astype(object)
        class_q.append([int(v) for v in h @ table[used]])
    S = d.S
    if n_na == 0:
        stats = [pc.statistic(S, Q, A, size) for A, size in zip(class_q, sizes)]
    else:
        n_used = sum(1 for n in sizes[0] if n > 0)
        stats = [(None, None, None, None, None, n_used - 1, S - n_used)] * len(labs)
    obs, Fs = stats[0], [s[0] for s in stats[1:]]
    n_ge = 0 if obs[0] is None else sum(1 for f in Fs if f is not None and f >= obs[0])
    return {
        "n_pairs": np.array([int(k.shape[0]), n_na], dtype=np.int64), "q_total": Q, "class_q": class_q, "sizes": sizes,
        "n_ge": n_ge, "n_undefined": sum(1 for f in Fs if f is None),
        "statistic": pc.to_double(obs[0]), "r2": pc.to_double(obs[1]),
        "pvalue": pc.na_real() if obs[0] is None else float(pc.Fraction(1 + n_ge, len(labs))),
        "ss_total": pc.to_double(obs[2]), "ss_within": pc.to_double(obs[3]), "ss_among": pc.to_double(obs[4]),
        "df_among": obs[5], "df_within": obs[6],
        "perm_statistic": np.array([pc.to_double(f) for f in Fs], dtype=np.float64),
        "class_size": np.array(sizes[0], dtype=np.int64),
        "class_ss": np.array([pc.to_double(pc.Fraction(a, n * pc.SCALE) if (n and n_na == 0) else None)
                              for a, n in zip(class_q[0], sizes[0])], dtype=np.float64),
    }


# ---- permdisp --------------------------------------------------------------------------------------------------------

_PERMDISP_ROWS = 256          # samples summed at a time: planes of [256, S] int64, never [S, S]


def _permdisp_sweep(d, cls, n_class):
    """(t_lo, t_hi [S, n_class] int64, both [2 m + 1] int64: the ordered valid pairs (a, b) per numerator, index
    num + m).  q is looked up per numerator (q_table; a pair that is not valid looks up one more entry, a 0); the
    columns are taken class by class (a stable sort of the labels), so one np.add.reduceat over the classes that have a
    sample sums every cell of a block of rows, whatever n_class is.  A cell has at most S - 1 < 2^16 limbs below 2^32:
    every sum is below 2^48."""
    S, m = d.S, d.K
    cls = np.asarray(cls, dtype=np.int64)
    assert cls.shape == (S,) and (S == 0 or (cls.min() >= 0 and cls.max() < n_class)) and S < 1 << 16
    table = [int(v) for v in q_table(d)] + [0]
    no_value = np.int32(2 * m + 1)
    limbs = (np.array([v & 0xFFFFFFFF for v in table], dtype=np.int64), np.array([v >> 32 for v in table], dtype=np.int64))
    order = np.argsort(cls, kind="stable")
    sizes = np.bincount(cls, minlength=n_class)
    used = np.nonzero(sizes)[0]
    starts = (np.cumsum(sizes) - sizes)[used]                        # strictly increasing: reduceat sums whole classes
    out = (np.zeros((S, n_class), dtype=np.int64), np.zeros((S, n_class), dtype=np.int64))
    both = np.zeros(2 * m + 2, dtype=np.int64)
    for a in range(0, S, _PERMDISP_ROWS):
        rows = slice(a, min(a + _PERMDISP_ROWS, S))
        k = np.take(np.where(d.valid[rows], d.key[rows] + np.int32(m), no_value), order, axis=1)
        both += np.bincount(k.ravel(), minlength=2 * m + 2)
        for limb, t in zip(limbs, out):
            t[rows, used] = np.add.reduceat(limb.take(k), starts, axis=1)
    assert all(int(t.max(initial=0)) < 1 << 48 for t in out)
    return out[0], out[1], both[:2 * m + 1]


def permdisp_limbs(d, cls, n_class):
    """(t_lo, t_hi [S, n_class] int64): per sample i and class c the sums of the low and of the high 32 bits of q over
    the samples j of class c whose pair with i is valid -- the two planes icikt_permdisp_f64 returns"""
    return _permdisp_sweep(d, cls, n_class)[:2]


def limbs_to_ints(lo, hi):
    """hi 2^32 + lo as an object array of Python ints; in int64 where that cannot overflow"""
    if hi.size == 0 or int(hi.max()) < 1 << 30:
        return ((hi << 32) + lo).astype(object)                      # (below 2^62 + 2^48)
    return hi.astype(object) * (1 << 32) + lo.astype(object)


def permdisp_table(d, cls, n_class):
    """tests/permdisp_checker.brute_table's tuple (n_values, n_na, Q, T, A, sizes) from the integers; T [S, n_class] is
    an object array of Python ints where the checker has a list of lists (T.tolist() is that list).  A pair that is
    not valid adds 0 and counts in n_na, and the table stays AS SUMMED when there is one (PERMANOVA's reference zeroes
    its class sums then).  Q is the pairs' histogram over the numerators times q_table, apart from the limb planes;
    A_c is half the sum of column c over the members of c."""
    S, m = d.S, d.K
    cls = np.asarray(cls, dtype=np.int64)
    t_lo, t_hi, both = _permdisp_sweep(d, cls, n_class)               # both: every pair twice, (a, b) and (b, a)
    T = limbs_to_ints(t_lo, t_hi)
    table = q_table(d)
    assert np.all(both % 2 == 0)
    n_val = int(both.sum()) // 2
    Q = sum(int(both[v]) // 2 * table[v] for v in np.nonzero(both)[0])
    assert 2 * Q == (int(t_hi.sum()) << 32) + int(t_lo.sum())        # (the planes' totals: below 2^63 and 2^51)
    A = [0] * n_class
    for c in np.unique(cls):
        twice = int(T[cls == c, c].sum())
        assert twice % 2 == 0
        A[int(c)] = twice // 2
    return n_val, S * (S - 1) // 2 - n_val, Q, T, A, [int(v) for v in np.bincount(cls, minlength=n_class)]


def permdisp(d, cls, n_class, labellings):
    """tests/permdisp_checker.brute_permdisp's dict: permdisp_table, then the checker's own tail (distances by 120-digit
    square roots, the ANOVA and the permutation test in Fractions)"""
    from tests.permdisp_checker import permdisp_tail
    n_val, n_na, Q, T, A, sizes = permdisp_table(d, cls, n_class)
    return permdisp_tail((n_val, n_na, Q, T.tolist(), A, sizes), cls, n_class, labellings)


# ---- p.adjust --------------------------------------------------------------------------------------------------------

def pvalue_keys(d, one_sided=False):
    """(keys: the distinct num -- |num| unless one_sided -- of the valid pairs, ascending; count per key; (i, j) of
    the first pair in combn order that has each key; n_na).  On the censored family the key is Design.pvalue_id: one
    integer per distinct (num, den, n_eff), what the p-value is a function of there."""
    i, j, _k, n_na = triangle(d)
    keys, first, count = np.unique(d.pvalue_id(i, j, one_sided), return_index=True, return_counts=True)
    return keys, count, i[first], j[first], n_na


def sorted_pvalues(d, p_of_key, one_sided=False):
    """(the tests' p-values ascending, a zero as +0; n_na): np.repeat of one p per distinct |num| (num when one_sided)
    by its count.  p_of_key: a p-value per key of pvalue_keys, in its order -- the p-value itself has no closed form
    here and comes from outside."""
    _keys, count, _i, _j, n_na = pvalue_keys(d, one_sided)
    p = np.asarray(p_of_key, dtype=np.float64) + 0.0
    assert p.shape == count.shape and not np.isnan(p).any()
    order = np.argsort(p, kind="stable")
    return np.repeat(p[order], count[order]), n_na


def unscanned(p, method):
    """the product a method's scan runs over, per sorted position: m p, (m + 1 - j) p or (m / j) p, capped at 1 -- the
    adjusted value BEFORE the running maximum or minimum (tests/padjust_checker.adjust_sorted_fast's operations)"""
    m = p.shape[0]
    if method == "bonferroni":
        u = float(m) * p
    elif method in ("holm", "hochberg"):
        u = np.arange(m, 0, -1).astype(np.float64) * p
    else:
        u = (float(m) / np.arange(1, m + 1).astype(np.float64)) * p
    return np.minimum(1.0, u)


def _runs(p):
    """(start, length) of the runs of equal p in the sorted p-values"""
    start = np.nonzero(np.concatenate([[True], p[1:] != p[:-1]]))[0]
    return start, np.diff(np.concatenate([start, [p.shape[0]]]))


def cuts_in_runs(p, method, alphas):
    """per alpha "inside", "edge" or None.  Equal p-values have equal adjusted values, so n_rejected never ends inside a
    run of equal p; what differs inside a run is the unscanned product.  "inside": some run of equal p holds products
    on both sides of alpha, so the running maximum or minimum alone decides where the whole run falls; "edge": no run
    does, and 0 < n_rejected < m: the products change sides where two runs meet; None: neither."""
    from tests.padjust_checker import adjust_sorted_fast
    adj, u = adjust_sorted_fast(p, method), unscanned(p, method)
    start, length = _runs(p)
    out = []
    for a in alphas:
        n = int(np.sum(adj <= a))
        below = np.add.reduceat((u <= a).astype(np.int64), start)
        if np.any((below > 0) & (below < length)):
            out.append("inside")
        else:
            out.append("edge" if 0 < n < p.shape[0] else None)
    return out


def alpha_inside_a_run(p, method):
    """a level that the unscanned products of the longest run of equal p straddle: the product at the run's middle
    (inside a run they fall strictly from place to place for holm, hochberg and BH while below the cap of 1).  None when
    no run has two products (bonferroni: m p is one value per run)."""
    u = unscanned(p, method)
    start, length = _runs(p)
    last = start + length - 1
    ok = u[start] != u[last]
    if not ok.any():
        return None
    r = int(np.argmax(np.where(ok, length, 0)))
    mid = int(start[r] + length[r] // 2)
    return float(u[mid]) if u[mid] < u[start[r]] else float(u[last[r]])


# ---- spanning forest -------------------------------------------------------------------------------------------------

def is_two_valued(d):
    if d.disc is None:
        return False
    ok = d.kind == VALID
    return bool(ok.any() and np.all(d.disc[ok] == d.disc[ok][0]))


def mst_two_valued(d):
    """tests/mst_checker.brute_mst's tuple in O(S) when every valid column is +-base: raw is +1 inside a sign group and
    -1 across.  Under the strict order (larger raw, then smaller combn index) the +1 edges come first, by (i, j):
    Kruskal takes every (g, x) from a group's smallest column g and nothing else inside the group, and the two stars
    come out in combn order.  Of the -1 edges the first in combn order, (the first valid column, the first column of
    the other sign), joins the two.  An NA column has no edge: a component of its own.  Every other design:
    brute_mst(d.raw)."""
    if not is_two_valued(d):
        from tests.mst_checker import brute_mst
        return brute_mst(d.raw)
    good = np.nonzero(d.kind == VALID)[0]
    first = d.sign[good[0]]
    groups = [good[d.sign[good] == first], good[d.sign[good] != first]]
    edges_ = sorted((int(g[0]), int(x)) for g in groups if len(g) for x in g[1:])
    if len(groups[1]):
        edges_.append((int(good[0]), int(groups[1][0])))
    ti = np.array([a for a, _b in edges_], dtype=np.int32)
    tj = np.array([b for _a, b in edges_], dtype=np.int32)
    component = np.empty(d.S, dtype=np.int32)                          # numbered by their smallest sample
    n_comp, tree = 0, -1
    for s in range(d.S):
        if d.kind[s] == VALID and tree >= 0:
            component[s] = tree
            continue
        if d.kind[s] == VALID:
            tree = n_comp
        component[s] = n_comp
        n_comp += 1
    assert len(ti) + n_comp == d.S
    return ti, tj, component, n_comp


# ---- the rectangle: the first Sq columns as the query, the rest as the reference ----------------------------------------

class Rect:
    """Q [n, Sq], R [n, Sr] F-ordered; num, valid [Sq, Sr]: no diagonal on a rectangle, a pair is valid iff neither
    column is an NA column; raw [Sq, Sr]: num / m, NaN where not valid; reasons [Sq, Sr]"""

    def __init__(self, d, Sq):
        assert 0 < Sq < d.S
        self.d, self.Sq, self.Sr = d, Sq, d.S - Sq
        self.Q, self.R = np.asfortranarray(d.X[:, :Sq]), np.asfortranarray(d.X[:, Sq:])
        self.num, self.valid = d.key[:Sq, Sq:], d.valid[:Sq, Sq:]
        self.raw = np.where(self.valid, d.value(self.num), np.nan)
        self.reasons = d.reasons()[:Sq, Sq:]

    def reason_counts(self):
        return np.bincount(self.reasons.ravel(), minlength=5).astype(np.int64)

    def max_taumax(self, queries=None):
        """the largest taumax of the rectangle alone (of the rows `queries` of it): not of the stacked triangle"""
        mask = np.zeros((self.d.S, self.d.S), dtype=bool)
        mask[np.arange(self.Sq) if queries is None else np.asarray(queries), self.Sq:] = True
        return self.d.max_taumax(mask)


def rect(d, Sq):
    return Rect(d, Sq)


def cross_topk(d, Sq, k):
    """topk's tuple for the rectangle: per query the k valid reference columns of largest num, ties by the smaller
    reference index; idx counts from the reference's first column"""
    r = rect(d, Sq)
    return _topk(d, r.num, r.valid, k)


def cross_class_table(d, Sq, ref_cls, n_class):
    """class_matrix's dict for the rectangle: cell (q, c) over the reference columns of class c that are valid with q"""
    r = rect(d, Sq)
    ref_cls = np.asarray(ref_cls)
    assert ref_cls.shape == (r.Sr,)
    return _class_cells(d, r.num, r.valid, ref_cls, n_class)
