"""The designed inputs on which the suite is pinned to the COMPILED reference (test infrastructure only), shared by
tests/golden/make_reference_golden.py, tests/test_oracle_vs_reference.py and tests/test_gpu_reference_parity.py.

Every matrix is built by integer arithmetic -- no random generator, so no numpy version can move a value: a column is
an affine map of the row index modulo a prime (distinct values in scattered order), divided by a power of two, with
tie groups and missing rows placed on an index permutation of the same kind.  Each is the smallest shape that reaches
its behaviour (the int32 sums of kendallc.cpp:112-114 and :267):

  step   n = 65, S = 6      one row past a 64-row step; ties, +-0, scattered NaN, rows missing in BOTH columns of some
                            pairs (local != global)
  t1     n = 1 500, S = 6   a value tie group of 1 100 rows: t(t-1)(2t+5) = 2 665 629 500 > 2^31; a column with 1 100
                            missing rows (the fill group is the wrapping group under "global"; under "local" the rows
                            it shares with column 4 go and it shrinks to 200); a heavily tied partner
  t0     n = 1 700, S = 4   a group of 1 300 rows: t(t-1)(t-2) = 2 191 932 600 > 2^31 as well, then the truncating / 2
  xtie   n = 46 500, S = 3  a group of 46 400 rows: t(t-1) = 2 152 913 600 > 2^31, xtie negative; a (value, fill) cell
                            of 46 350 rows wraps `ntie` too; these columns run in the whole-wave kernels
  and the degenerate pairs: all missing, constant, one row, two rows, constant only after the fill or the local removal.

"Ties equal the total" (reason 4, kendallc.cpp:291) has no input of its own below 65 536 rows: sum t(t-1) over the
groups is below n(n-1) < 2^32 unless one group holds every row, and that is "single unique value" (reason 3) three
statements earlier; a wrapped sum is negative or smaller.  The constant columns are the nearest there is.
"""
import collections
import functools
import hashlib
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_ici_kt.npz")
MATRIX_NAMES = ("step", "t1", "t0", "xtie")

PERSPECTIVES = ("local", "global")               # index = oracle.PERSPECTIVES' code
ALTERNATIVES = ("two.sided", "less", "greater")
CONTINUITY = (False, True)
COUNT_FIELDS = ("n", "missing", "dis", "ntie", "xtie", "ytie", "x0", "x1", "y0", "y1", "tot", "sum_obs")
NAN = float("nan")

Matrix = collections.namedtuple("Matrix", "name X stored wraps")


def scatter(n, a, p, b=0):
    """(a i + b) mod p for i < n <= p, p prime, 0 < a < p: n distinct integers in scattered order (int64)."""
    assert n <= p and 0 < a < p
    return (np.arange(n, dtype=np.int64) * a + b) % p


def shuffle(n, a, p):
    """A permutation of 0 .. n-1: the rows in the order of scatter(n, a, p)."""
    return np.argsort(scatter(n, a, p), kind="stable")


def _col(n, a, p, div=8.0, shift=0):
    return (scatter(n, a, p) - shift).astype(np.float64) / div


def _step():
    n = 65
    X = np.empty((n, 6), dtype=np.float64)
    X[:, 0] = _col(n, 29, 67, 8.0, 33)                          # distinct, both signs
    X[:, 1] = (scatter(n, 23, 67) % 9 - 4).astype(np.float64)   # nine values, 0 among them
    X[shuffle(n, 5, 67)[:3], 1] = -0.0                          # -0.0 ties with +0.0
    X[:, 2] = _col(n, 31, 71, 4.0)
    X[:, 3] = (scatter(n, 37, 71) % 5).astype(np.float64)
    miss = scatter(n, 13, 67) % 5 == 0
    X[miss, 2] = NAN
    X[miss | (np.arange(n) % 11 == 3), 3] = NAN                 # column 2's missing rows and six more
    X[:, 4] = _col(n, 41, 73, 2.0, 36)
    X[:20, 4] = NAN
    X[:, 5] = (scatter(n, 17, 73) % 2).astype(np.float64)       # two values
    X[10:41, 5] = NAN                                           # rows 10 .. 19 are missing in column 4 too
    return Matrix("step", X, True, False)


def _t1():
    n, g = 1500, 1100
    X = np.empty((n, 6), dtype=np.float64)
    X[:, 0] = _col(n, 577, 1511)
    X[shuffle(n, 211, 1511)[:g], 0] = 0.5625                     # the value group of 1 100 rows
    X[:, 1] = _col(n, 733, 1523)
    m1 = shuffle(n, 389, 1523)
    X[m1[:g], 1] = NAN                                          # 1 100 missing rows
    X[:, 2] = (scatter(n, 997, 1531) % 3).astype(np.float64)    # three values of about 500 rows each
    X[:, 3] = _col(n, 1013, 1543, 16.0)
    X[scatter(n, 61, 1543) % 10 == 0, 3] = NAN
    X[:, 4] = _col(n, 401, 1549, 4.0, 700)
    X[m1[:900], 4] = NAN                                        # 900 of column 1's missing rows ...
    X[m1[g:g + 200], 4] = NAN                                   # ... and 200 of its present ones
    X[:, 5] = _col(n, 859, 1553)
    return Matrix("t1", X, True, True)


def _t0():
    n, g = 1700, 1300
    X = np.empty((n, 4), dtype=np.float64)
    X[:, 0] = _col(n, 641, 1709, 8.0, 850)
    X[shuffle(n, 277, 1709)[:g], 0] = -2.3125
    X[:, 1] = _col(n, 809, 1721)
    X[shuffle(n, 503, 1721)[:g], 1] = NAN
    X[:, 2] = (scatter(n, 1117, 1723) % 4).astype(np.float64)
    X[:, 3] = _col(n, 947, 1733, 32.0)
    X[scatter(n, 71, 1733) % 8 == 0, 3] = NAN
    return Matrix("t0", X, True, True)


def _xtie():
    n, g = 46500, 46400
    X = np.empty((n, 3), dtype=np.float64)
    X[:, 0] = _col(n, 17389, 46507)
    rows = shuffle(n, 7919, 46507)
    X[rows[:g], 0] = 1.3125
    X[:, 1] = _col(n, 30011, 46511, 4.0)
    X[rows[50:50 + g], 1] = NAN                                 # 46 350 rows shared with column 0's group
    X[:, 2] = (scatter(n, 11683, 46523) // 2).astype(np.float64)   # pairs of equal values
    return Matrix("xtie", X, False, True)


@functools.lru_cache(maxsize=None)
def matrices():
    out = (_step(), _t1(), _t0(), _xtie())
    for m in out:
        m.X.setflags(write=False)
    return out


def matrix(name):
    return {m.name: m for m in matrices()}[name]


def pairs_of(S):
    pi, pj = np.triu_indices(S, k=1)
    return pi.astype(np.int32), pj.astype(np.int32)


def digest(X):
    """The matrix's bytes (column-major float64) as a SHA-256 hex string: the fixture holds it for the matrix that is
    rebuilt, not stored."""
    return hashlib.sha256(np.asfortranarray(X, dtype=np.float64).tobytes(order="F")).hexdigest()


def degenerates():
    """(name, x, y) of the degenerate pairs."""
    a = np.array
    return (
        ("all_missing_x", a([NAN, NAN, NAN]), a([1.0, 2.0, 3.0])),
        ("all_missing_both", a([NAN, NAN]), a([NAN, NAN])),
        ("all_missing_after_local", a([NAN, NAN, 1.0]), a([NAN, NAN, NAN])),
        ("constant_x", a([1.0, 1.0, 1.0]), a([1.0, 2.0, 3.0])),
        ("constant_y", a([3.0, 1.0, 2.0, 5.0]), a([0.0, -0.0, 0.0, 0.0])),
        ("constant_after_local", a([1.0, 1.0, NAN, 1.0]), a([1.0, 2.0, NAN, 3.0])),
        ("fill_makes_two_values", a([NAN, NAN, 1.0]), a([1.0, 2.0, 3.0])),
        ("one_row", a([1.0]), a([2.0])),
        ("one_row_after_local", a([1.0, NAN]), a([2.0, NAN])),
        ("zero_rows", a([]), a([])),
        ("two_rows", a([1.0, 2.0]), a([2.0, 1.0])),
        ("two_rows_crossed_na", a([1.0, NAN]), a([NAN, 2.0])),
        ("two_rows_tied_x", a([1.0, 1.0]), a([1.0, 2.0])),
        ("three_rows", a([1.0, 2.0, 3.0]), a([1.0, 3.0, 2.0])),
    )


def exact_tie_sums(col):
    """(tie, t0, t1) of a filled column in Python integers: the sums of kendallc.cpp:112-114 without the int32."""
    t = [int(c) for c in np.unique(col, return_counts=True)[1]]
    return (sum(c * (c - 1) for c in t) // 2, sum(c * (c - 1) * (c - 2) for c in t) // 2,
            sum(c * (c - 1) * (2 * c + 5) for c in t))


def exact_joint_ties(x2, y2):
    """ntie of two filled columns in Python integers (kendallc.cpp:267 without the int32)."""
    cells = np.unique(np.stack([x2, y2], axis=1), axis=0, return_counts=True)[1]
    return sum(int(c) * (int(c) - 1) // 2 for c in cells)


def fill(x, y, perspective):
    """The two columns as kendallc.cpp:180-219 leaves them: "local" drops the rows missing in both, then every NaN is
    its column's minimum - 0.1.  None where a column has no value left."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if perspective == "local":
        keep = ~(np.isnan(x) & np.isnan(y))
        x, y = x[keep], y[keep]
    if np.isnan(x).all() or np.isnan(y).all():
        return None
    return (np.where(np.isnan(x), x[~np.isnan(x)].min() - 0.1, x), np.where(np.isnan(y), y[~np.isnan(y)].min() - 0.1, y))


def in_int32_regime(x, y, perspective):
    """Whether one of the reference's int sums leaves int32 on this pair, from the group sizes in Python integers:
    sum t(t-1), sum t(t-1)(t-2) or sum t(t-1)(2t+5) of a column, a joint cell's c(c-1), or the sum of c(c-1)/2.  The
    terms are non-negative, so nothing wraps on the way unless the total does; and a wrapped total differs from the
    exact one by a multiple of 2^32, so below this line the two readings of the code cannot be told apart and from it
    on they must be."""
    cols = fill(x, y, perspective)
    if cols is None or cols[0].shape[0] < 2:
        return False
    top = 0
    for col in cols:
        tie, t0, t1 = exact_tie_sums(col)
        top = max(top, 2 * tie, 2 * t0, t1)            # (both halved sums are even: the halves lose nothing)
    cells = np.unique(np.stack(cols, axis=1), axis=0, return_counts=True)[1]
    top = max(top, max(int(c) * (int(c) - 1) for c in cells), exact_joint_ties(*cols))
    return top >= 2 ** 31


# ---- the committed fixture (tests/golden/make_reference_golden.py says what it holds) --------------------------------
@functools.lru_cache(maxsize=None)
def load_fixture():
    with np.load(FIXTURE) as z:
        fx = {k: z[k] for k in z.files}
    for a in fx.values():
        a.setflags(write=False)
    return fx


def fixture_matrix(fx, name):
    """The matrix the fixture's answers belong to: the stored one, or the rebuilt one after its digest is checked."""
    if f"X_{name}" in fx:
        return fx[f"X_{name}"]
    X = matrix(name).X
    assert digest(X) == str(fx[f"sha256_{name}"]), f"the rebuilt matrix {name} is not the one the fixture was made from"
    return X


def fixture_degenerates(fx):
    return [(str(name), fx["deg_x"][k, :n], fx["deg_y"][k, :n])
            for k, (name, n) in enumerate(zip(fx["deg_names"], fx["deg_len"]))]
