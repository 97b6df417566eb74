"""Exact reference of the ICI-Kt epilogue (test infrastructure only): counts -> tau, tau_max, completeness, variance,
z and the p-value at 60 digits in mpmath, and the committed case set that walks z through every branch of R's pnorm
(Cody 1969), both tails, up to and beyond its cut-off at |z| = 37.5193.

The p-value's yardstick is the SCALED error |got - p| / p / ((1 + z^2) 2^-52): a relative error of z of one unit
roundoff moves a tail p by about z^2 units, so the measure is about 1 for correctly rounded double arithmetic anywhere
on the axis, and a wrong digit in a coefficient table shows as hundreds or more (profiles/epilogue_tails.md)."""
import collections
import functools

import mpmath
import numpy as np

DPS = 60
UNIT = 2.0 ** -52
# the branch edges of pnorm_both as the doubles the code compares with
EDGE_SMALL = 0.67448975
EDGE_MIDDLE = 5.656854249492380195206754896838
CUTOFF = 37.5193
EDGES = (EDGE_SMALL, EDGE_MIDDLE, CUTOFF)
BRANCHES = ("small", "middle", "tail", "cut")
ALTERNATIVES = ("two.sided", "less", "greater")
COUNT_FIELDS = ("n", "missing", "dis", "ntie", "xtie", "ytie", "x0", "x1", "y0", "y1", "tot")

# The CPU oracle's worst scaled error, measured 2026-10-17 with
#     python -m pytest tests/test_epilogue_reference.py -q -s
# (gcc 13 -O2 -ffp-contract=off, glibc libm, x86-64): "grid" over the pnorm grid, "cases" over cases() under every
# alternative, continuity and int32_compat setting.  The CPU test asserts <= 2 E_CPU (another libm or compiler), the
# device test <= 4 E_CPU (tests/test_gpu_epilogue_tails.py says why 4).
E_CPU = {"grid": 1.04, "cases": 1.05}

Exact = collections.namedtuple("Exact", "tau tau_max completeness var s_adj z p")
Case = collections.namedtuple("Case", "name X pi pj perspectives d")


def perm_with_inversions(n, d):
    """A permutation of 0..n-1 (float64) with exactly d inversions: the greedy Lehmer code, position i takes as many
    of the remaining inversions as it can hold (n - 1 - i).  With x = arange(n) the pair has dis = d."""
    tot = n * (n - 1) // 2
    if not 0 <= d <= tot:
        raise ValueError(f"d = {d} outside [0, {tot}]")
    # the code is n-1, n-2, ... on the first k positions (they hold n-1, n-2, ... n-k), r < n-k-1 on the next (it
    # holds the r-th smallest value left) and 0 from there on (the rest in ascending order)
    k = int(np.searchsorted(np.cumsum(n - 1 - np.arange(n)), d, side="right")) if d < tot else n
    out = np.empty(n, dtype=np.float64)
    out[:k] = n - 1 - np.arange(k)
    if k < n:
        r = d - k * (2 * n - k - 1) // 2
        out[k] = r
        out[k + 1:] = np.delete(np.arange(n - k), r)
    return out


def pair_counts(x, y, perspective="global"):
    """The eleven integer count fields of one pair in plain numpy (O(n^2) for dis), exact in int64: the reference's
    NA handling (kendallc.cpp:180-219), no int32 wrap (none can happen below 1291 rows)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if perspective == "local":
        keep = ~(np.isnan(x) & np.isnan(y))
        x, y = x[keep], y[keep]
    n = x.shape[0]
    missing = int((np.isnan(x) | np.isnan(y)).sum())
    x = np.where(np.isnan(x), np.nanmin(x) - 0.1, x)
    y = np.where(np.isnan(y), np.nanmin(y) - 0.1, y)

    def ties(t):
        return (int((t * (t - 1)).sum()) // 2, int((t * (t - 1) * (t - 2)).sum()) // 2,
                int((t * (t - 1) * (2 * t + 5)).sum()))
    rx, cx = np.unique(x, return_inverse=True, return_counts=True)[1:]       # dense ranks and group sizes (int64)
    ry, cy = np.unique(y, return_inverse=True, return_counts=True)[1:]
    xtie, x0, x1 = ties(cx)
    ytie, y0, y1 = ties(cy)
    cells = np.unique(rx * cy.shape[0] + ry, return_counts=True)[1]
    ntie = int((cells * (cells - 1)).sum()) // 2
    rx, ry = rx.astype(np.int32), ry.astype(np.int32)
    dis = int(np.count_nonzero((rx[:, None] < rx[None, :]) & (ry[:, None] > ry[None, :])))
    return (n, missing, dis, ntie, xtie, ytie, x0, x1, y0, y1, n * (n - 1) // 2)


@functools.lru_cache(maxsize=None)
def _exact_core(counts, continuity):
    n, missing, dis, ntie, xtie, ytie, x0, x1, y0, y1, tot = counts
    if n < 3 or xtie == tot or ytie == tot:
        raise ValueError("no epilogue for this pair (n < 3 or ties equal the total)")
    with mpmath.workdps(DPS):
        mpf = mpmath.mpf
        den = mpmath.sqrt(mpf(tot - xtie) * mpf(tot - ytie))                 # kendallc.cpp:300-303
        s = tot - xtie - ytie + ntie - 2 * dis
        tau = mpf(s) / den
        tau_max = mpf(tot - xtie - ytie + ntie) / den                       # not clipped
        m = n * (n - 1)
        s_adj = mpf(s)                                                      # tau sqrt((m/2 - xtie)(m/2 - ytie)), m/2 = tot
        if abs(tau) > 1:                                                    # :304-308
            tau = mpf(1 if tau > 0 else -1)
            s_adj = tau * den
        var = (mpf(m * (2 * n + 5) - x1 - y1) / 18 + mpf(2 * xtie * ytie) / m
               + mpf(x0 * y0) / (9 * m * (n - 2)))                          # :311-312
        if continuity:                                                      # :315-319, sign(0) = 0
            s_adj = mpmath.sign(s_adj) * (abs(s_adj) - 1)
        z = s_adj / mpmath.sqrt(var)
        if abs(z) >= mpf(CUTOFF):                                           # R's pnorm: the vanishing tail is 0
            small, big = mpf(0), mpf(1)
        else:
            small = mpmath.erfc(abs(z) / mpmath.sqrt(2)) / 2
            big = 1 - small
        lower, upper = (small, big) if z < 0 else (big, small)
        return tau, tau_max, 1 - mpf(missing) / n, var, s_adj, z, lower, upper


def exact_epilogue(counts, alternative, continuity):
    """kendallc.cpp:300-335 on the eleven integer counts at 60 digits, with R's cut-off.  Every field is an mpf."""
    tau, tau_max, comp, var, s_adj, z, lower, upper = _exact_core(tuple(int(c) for c in counts), bool(continuity))
    with mpmath.workdps(DPS):
        p = {"less": lower, "greater": upper, "two.sided": 2 * min(lower, upper)}[alternative]
    return Exact(tau, tau_max, comp, var, s_adj, z, p)


def exact_pnorm(z, lower_tail=True):
    """R's pnorm(z) of a double z at 60 digits, with the cut-off (and +-inf)."""
    with mpmath.workdps(DPS):
        if z == 0:
            return mpmath.mpf(0.5)
        if abs(z) >= CUTOFF:
            small, big = mpmath.mpf(0), mpmath.mpf(1)
        else:
            small = mpmath.erfc(abs(mpmath.mpf(z)) / mpmath.sqrt(2)) / 2
            big = 1 - small
        return small if (z < 0) == bool(lower_tail) else big      # the tail that vanishes, or the other


def scaled_error(got, p, z):
    """|got - p| / p / ((1 + z^2) 2^-52) as a float (p > 0)."""
    with mpmath.workdps(DPS):
        return float(abs(mpmath.mpf(float(got)) - p) / p / ((1 + mpmath.mpf(z) ** 2) * UNIT))


def branch_of(z):
    a = abs(float(z))
    return "small" if a <= EDGE_SMALL else "middle" if a <= EDGE_MIDDLE else "tail" if a < CUTOFF else "cut"


def ulps(got, exact):
    """|got - exact| in units of the spacing of doubles at exact."""
    with mpmath.workdps(DPS):
        return float(abs(mpmath.mpf(float(got)) - exact) / float(np.spacing(abs(float(exact)) or 1.0)))


TINY = 2.0 ** -1022          # the smallest normal double
TAU_ULPS = 4
COMPLETENESS_ULPS = 1


def check_call(out, counts, alternative, continuity, bound, label=""):
    """One call's four doubles (out [P, 4]: tau, p, tau_max, completeness) against exact_epilogue of its integer counts
    ([P, >= 11]).  Asserts: p exactly 0.0 / 1.0 beyond the cut-off; p exactly 0.5, 0.5, 1.0 where continuity brings
    S = 0 or |S| = 1 to s_adj = 0; p's scaled error <= bound where p is a normal double, and |got - p| <=
    bound (1 + z^2) 2^-52 p + 4 2^-1074 below; tau and tau_max within 4 ulp, completeness within 1.  Returns the worst
    figures: {"p": {branch: scaled error}, "tau": ulps, "tau_max": ulps, "completeness": ulps}."""
    worst = {"p": dict.fromkeys(BRANCHES, 0.0), "tau": 0.0, "tau_max": 0.0, "completeness": 0.0}
    bad = []
    for k in range(out.shape[0]):
        c = tuple(int(v) for v in counts[k][:len(COUNT_FIELDS)])
        ex = exact_epilogue(c, alternative, continuity)
        tau, p, tau_max, comp = (float(v) for v in out[k])
        where = f"{label} pair {k} z={float(ex.z):.6g}"
        s = c[10] - c[4] - c[5] + c[3] - 2 * c[2]
        branch = branch_of(ex.z)
        if not 0.0 <= p <= 1.0:
            bad.append(f"{where}: p = {p!r}")
        elif branch == "cut":
            if p != float(ex.p):
                bad.append(f"{where}: p = {p!r} beyond the cut-off, not {float(ex.p)}")
        elif ex.p >= TINY:
            e = scaled_error(p, ex.p, ex.z)
            worst["p"][branch] = max(worst["p"][branch], e)
            if not e <= bound:
                bad.append(f"{where}: p = {p!r}, exact {float(ex.p)!r}, scaled error {e:.4g} > {bound}")
        else:
            with mpmath.workdps(DPS):
                if not abs(mpmath.mpf(p) - ex.p) <= bound * (1 + ex.z ** 2) * UNIT * ex.p + 4 * mpmath.mpf(2) ** -1074:
                    bad.append(f"{where}: subnormal p = {p!r}, exact {float(ex.p)!r}")
        if continuity and abs(s) <= 1 and p != {"two.sided": 1.0}.get(alternative, 0.5):
            bad.append(f"{where}: S = {s} under continuity gives p = {p!r}")
        for name, got, want, lim in (("tau", tau, ex.tau, TAU_ULPS), ("tau_max", tau_max, ex.tau_max, TAU_ULPS),
                                     ("completeness", comp, ex.completeness, COMPLETENESS_ULPS)):
            u = ulps(got, want) if want != 0 else (0.0 if got == 0 else float("inf"))
            worst[name] = max(worst[name], u)
            if not u <= lim:
                bad.append(f"{where}: {name} = {got!r}, exact {float(want)!r}, {u:.3g} ulp > {lim}")
    assert not bad, f"{len(bad)} failures, first: " + "; ".join(bad[:5])
    return worst


def merge_worst(into, worst):
    for k, v in worst.items():
        if isinstance(v, dict):
            merge_worst(into.setdefault(k, {}), v)
        else:
            into[k] = max(into.get(k, 0.0), v)
    return into


# ---- the committed case set -----------------------------------------------------------------------------------------
def _plain_cols(n):
    return np.arange(n, dtype=np.float64), lambda d: perm_with_inversions(n, d)


def _tied_cols(n):
    def y(d):
        v = np.floor(perm_with_inversions(n, d) / 2)
        v[:n // 10] = np.nan
        return v
    return np.floor(np.arange(n, dtype=np.float64) / 3), y


def _local_cols(n):
    x = np.arange(n, dtype=np.float64)
    x[:40] = np.nan

    def y(d):
        v = perm_with_inversions(n, d)
        v[10:60] = np.nan                      # rows 10..39 are missing in both columns
        return v
    return x, y


def _d_values(n, zfun, n_even, n_log, must_reach):
    """The d values of one matrix: the ends and the middle, n_even evenly spaced, n_log log-spaced toward tot / 2 on
    both sides, and for each sign of z, each branch edge and continuity off / on the two d on either side of the edge
    whose exact z is nearest to it (never within 1e-9 of it).  An edge beyond the matrix's reach is an error where
    must_reach (the plain matrix reaches |z| = 47) and is left out elsewhere: with the rows of its largest values
    missing, a fully reversed column of the tied matrix stops at z = -30."""
    tot = n * (n - 1) // 2
    half = tot // 2
    ds = {0, 1, 2, half - 1, half, half + 1, tot - 1, tot}
    ds.update(int(v) for v in np.round(np.linspace(0, tot, n_even)))
    off = np.unique(np.round(np.logspace(0, np.log10(half), n_log // 2)).astype(np.int64))
    ds.update(int(half - o) for o in off)
    ds.update(int(half + o) for o in off)
    for continuity in (False, True):
        for sign in (1.0, -1.0):
            for edge in EDGES:
                target = sign * edge
                lo, hi = 0, tot                              # z falls as d grows: first d with z(d) < target
                if not zfun(lo, continuity) > target > zfun(hi, continuity):
                    if must_reach:
                        raise ValueError(f"z = {target} is out of this matrix's reach")
                    continue
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    if zfun(mid, continuity) < target:
                        hi = mid
                    else:
                        lo = mid
                near = [(zfun(d, continuity) - target, d) for d in range(max(0, hi - 6), min(tot, hi + 6) + 1)]
                above = sorted((dz, d) for dz, d in near if dz > 1e-9)[:2]
                below = sorted((-dz, d) for dz, d in near if dz < -1e-9)[:2]
                if len(above) < 2 or len(below) < 2:
                    raise ValueError(f"no d on both sides of z = {target}")
                ds.update(d for _dz, d in above + below)
    return sorted(ds)


def _matrix(name, n, cols, perspectives, n_even, n_log, rng):
    x, yfun = cols(n)

    @functools.lru_cache(maxsize=None)
    def zfun(d, continuity):
        if cols is _plain_cols:
            counts = (n, 0, d, 0, 0, 0, 0, 0, 0, 0, n * (n - 1) // 2)
        else:
            counts = pair_counts(x, yfun(d), perspectives[-1])
        return float(exact_epilogue(counts, "less", continuity).z)
    ds = _d_values(n, zfun, n_even, n_log, cols is _plain_cols)
    return _assemble(name, x, yfun, ds, perspectives, rng)


def _assemble(name, x, yfun, ds, perspectives, rng):
    X = np.empty((x.shape[0], 1 + len(ds)), dtype=np.float64, order="F")
    X[:, 0] = x
    for j, d in enumerate(ds):
        X[:, 1 + j] = yfun(d)
    X = np.asfortranarray(X[rng.permutation(x.shape[0])])       # the rows in no particular order: same counts
    X.setflags(write=False)
    pj = np.arange(1, 1 + len(ds), dtype=np.int32)
    pi = np.zeros_like(pj)
    pi.setflags(write=False)
    pj.setflags(write=False)
    return Case(name, X, pi, pj, perspectives, tuple(ds))


@functools.lru_cache(maxsize=None)
def cases():
    """The committed case set: column 0 is x, every further column one permutation, the pair list is (0, j)."""
    rng = np.random.default_rng(20261017)
    out = [_matrix("plain", 1000, _plain_cols, ("global",), 160, 120, rng),
           _matrix("tied", 1000, _tied_cols, ("global",), 160, 120, rng),
           _matrix("local", 700, _local_cols, ("global", "local"), 60, 40, rng)]
    for n in (3, 4, 5, 8, 40):
        x, yfun = _plain_cols(n)
        out.append(_assemble(f"small{n}", x, yfun, range(n * (n - 1) // 2 + 1), ("global",), rng))
    return tuple(out)
