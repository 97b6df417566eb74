"""The yardstick of cor_fast's Student-t p-values (tests/t_tail_exact.py) against things it shares no code with, and
against it: ``api.cor_test_pvalue`` and the numpy path on the designed lattice (tests/cor_lattice.py), and the Python
transcription of the device functions (tests/cor_t_port.py) on a dense (df, t) grid, with its iteration count and the
mutations the bars catch.  The figures these tests print are recorded in profiles/cor_t_tail.md."""
import math

import mpmath
import numpy as np
import pytest
from scipy import stats

from icikendalltau_amd import _lib, api
from tests import cor_lattice as L
from tests.cor_t_port import MUTATIONS, Port
from tests.t_tail_exact import ALTERNATIVES, DPS, t_pvalue_exact, t_tail_exact, t_tail_exact_t

DFS = (1, 2, 3, 5, 9, 10, 18, 19, 20, 21, 22, 40, 100, 1000, 1288, 1289, 20000, 65533, 262142)


# ---- the reference itself -----------------------------------------------------------------------------------------

def _digits(got, want):
    return float(-mpmath.log10(abs(got / want - 1))) if got != want else math.inf


def test_closed_forms_at_400_digits():
    """df = 1: 1/2 - atan(t) / pi.  df = 2: 1/2 - t / (2 sqrt(2 + t^2)).  From t and from rho."""
    ts = [0.0, 1e-300, 1e-9, 0.3, 1.0, 1 + 1e-12, 1.7, 12.0, 1e5, 1e9, 1e150]
    rhos = [0.0, 1e-200, 3e-9, 0.25, -0.5, math.sqrt(0.5), 0.9, -(1 - 2.0 ** -20), 1 - 2.0 ** -40, 1.0, -1.0]
    worst = math.inf
    with mpmath.workdps(DPS + 700):          # the closed forms cancel: 300 digits at t = 1e150
        for t in ts:
            tm = mpmath.mpf(t)
            worst = min(worst, _digits(t_tail_exact_t(t, 1), mpmath.mpf(1) / 2 - mpmath.atan(tm) / mpmath.pi))
            worst = min(worst, _digits(t_tail_exact_t(t, 2), mpmath.mpf(1) / 2 - tm / (2 * mpmath.sqrt(2 + tm * tm))))
        for rho in rhos:
            r = abs(mpmath.mpf(rho))
            if r == 1:
                assert t_tail_exact(rho, 1) == 0 and t_tail_exact(rho, 2) == 0
                continue
            tm = r / mpmath.sqrt(1 - r * r)
            worst = min(worst, _digits(t_tail_exact(rho, 1), mpmath.mpf(1) / 2 - mpmath.atan(tm) / mpmath.pi))
            tm *= mpmath.sqrt(2)
            worst = min(worst, _digits(t_tail_exact(rho, 2), mpmath.mpf(1) / 2 - tm / (2 * mpmath.sqrt(2 + tm * tm))))
    print(f"closed forms: {worst:.0f} digits at least")
    assert worst >= DPS


def test_alternatives():
    with mpmath.workdps(DPS + 100):
        def same(a, b):
            return abs(a - b) <= mpmath.mpf(10) ** -DPS

        for rho in (0.3, -0.3):
            tail = t_tail_exact(rho, 7)
            assert same(t_pvalue_exact(rho, 7, "two.sided"), 2 * tail)
            assert t_pvalue_exact(rho, 7, "less" if rho < 0 else "greater") == tail
            assert same(t_pvalue_exact(rho, 7, "greater" if rho < 0 else "less"), 1 - tail)
        assert t_pvalue_exact(0.0, 7, "less") == t_pvalue_exact(0.0, 7, "greater") == mpmath.mpf(1) / 2
    with pytest.raises(ValueError):
        t_pvalue_exact(0.1, 7, "both")
    with pytest.raises(ValueError):
        t_tail_exact(0.1, 2.5)


def _t_grid(df):
    """About 130 |t| from 0 to 1e9: quarter decades, the centre, the far tail of long columns (10 < t < 37.5), and
    the continued fraction's swap point x = (a + 1) / (a + b + 2), t^2 = 3 df / (df + 2), times 1 and 1 +- 1e-12."""
    sw = math.sqrt(3.0 * df / (df + 2.0))
    ts = {0.0, sw, sw * (1 + 1e-12), sw * (1 - 1e-12)}
    ts.update(float(v) for v in 10.0 ** np.linspace(-9, 9, 73))
    ts.update(float(v) for v in np.linspace(0.15, 8.0, 30))
    ts.update(float(v) for v in np.linspace(10.5, 37.5, 24))
    return sorted(ts)


_GRID = []


def _grid():
    """(df, t, exact tail) wherever the tail is >= 1e-300 or t^2 >= df (where the series is short whatever the tail;
    the rest, p < 1e-300 at t^2 < df, costs the reference a term per unit of df and tells nothing more)."""
    if not _GRID:
        for df in DFS:
            for t in _t_grid(df):
                if stats.t.sf(t, df) >= 1e-300 or t * t >= df:
                    _GRID.append((df, t, t_tail_exact_t(t, df)))
    return _GRID


def test_against_scipy_t_sf():
    """scipy.stats.t.sf to 1e-12 relative wherever p >= 1e-290 (it measures 1.5e-13)."""
    worst, at, count = 0.0, None, 0
    for df, t, ref in _grid():
        sf = float(stats.t.sf(t, df))
        if sf >= L.P_FLOOR:
            count += 1
            rel = abs(float(sf / ref - 1))
            if rel > worst:
                worst, at = rel, (df, t)
    print(f"scipy.stats.t.sf against the series: worst relative {worst:.3g} at (df, t) = {at} over {count} points")
    assert count > 1500 and worst <= 1e-12


# ---- the lattice and the front end's restatement on it --------------------------------------------------------------

@pytest.mark.parametrize("n", L.PEARSON_N)
def test_lattice_is_where_it_says(n):
    """By the reference alone: every designed point has p >= 1e-289 (two-sided; a tail is half of it), the named
    underflow points lie below the floor, and every n holds the centre on both sides of the swap point."""
    df = n - 2
    tg = L.pearson_targets(n)
    assert len(tg) <= 40 and {t.rho for t in tg} == {-t.rho for t in tg}
    for t in tg:
        p = t_pvalue_exact(t.rho, df)
        if t.underflow:
            assert p < L.P_FLOOR / 1e10, (t, float(p))
        else:
            assert p >= 0.99e-289 and abs(t.rho) < 1, (t, float(p))
    xs = [1 - t.rho ** 2 for t in tg]
    sw = (df + 2.0) / (df + 5.0)
    assert any(sw < x < sw * (1 + 1e-8) for x in xs) and any(sw * (1 - 1e-8) < x < sw for x in xs)
    assert any(t.underflow and abs(t.rho) == 1 for t in tg)
    if n >= 1291:
        assert any(t.underflow and abs(t.rho) < 1 for t in tg)
        assert sum(not t.underflow for t in tg) == 2 * (len(L.P_TARGETS) + 2)


@pytest.mark.parametrize("alternative", ALTERNATIVES)
def test_front_end_pearson_on_the_lattice(alternative):
    """api.cor_test_pvalue, which the device is said to restate, at the designed rho themselves."""
    for n in L.PEARSON_N:
        tg = L.pearson_targets(n)
        rho = [t.rho for t in tg]
        pv = [api.cor_test_pvalue(r, n, "pearson", alternative) for r in rho]
        L.compare_with_exact(rho, pv, n - 2, alternative, [not t.underflow for t in tg], "cor_test_pvalue pearson")


@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("n", [k for k in L.PEARSON_N if k <= 20002])
def test_numpy_path_pearson_lattice(n, pad):
    """From columns to p through the front end's numpy path: the lattice's columns do have the designed rho."""
    tg = L.pearson_targets(n)
    X, pi, pj = L.pearson_lattice(n, tg, pad)
    assert X.shape == (n + pad, len(tg) + 1)
    for alternative in ALTERNATIVES:
        out, rsn = api._cor_pairs_numpy(X, pi, pj, "pearson", bool(pad), alternative, False)
        assert (rsn == _lib.COR_OK).all() and (out[:, 2] == n).all()
        assert np.abs(out[:, 0] - [t.rho for t in tg]).max() <= 1e-9
        L.compare_with_exact(out[:, 0], out[:, 1], n - 2, alternative, [not t.underflow for t in tg],
                             f"numpy path pearson pad={pad}")


@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("n,tied", L.SPEARMAN_CASES)
def test_numpy_path_spearman_lattice(n, tied, pad):
    """Spearman with ties, or at n >= 1290: cor_test_pvalue's t branch at the rho of designed rank columns; every
    point is >= 1e-290 by the reference alone, and the columns reach both tails and the centre."""
    X, pi, pj = L.spearman_lattice(n, tied, pad)
    for alternative in ALTERNATIVES:
        out, rsn = api._cor_pairs_numpy(X, pi, pj, "spearman", bool(pad), alternative, False)
        assert (rsn == (_lib.COR_TIES if tied and n < 1290 else _lib.COR_OK)).all() and (out[:, 2] == n).all()
        L.compare_with_exact(out[:, 0], out[:, 1], n - 2, alternative, [True] * len(pi),
                             f"numpy path spearman tied={tied} pad={pad}")
    L.assert_spearman_spread(out[:, 0], n)


# ---- the transcription of the device functions ----------------------------------------------------------------------

def _port_errors(port, keep=None):
    """{df: (worst relative error where the tail is >= 1e-290, its t, worst |d|)} of 2 t_tail over the grid, or over
    its points (df, t) that keep() takes."""
    out = {}
    for df, t, ref in _grid():
        if keep is not None and not keep(df, t):
            continue
        got = 2.0 * port.t_tail(t, float(df))
        w = out.setdefault(df, [0.0, None, 0.0])
        w[2] = max(w[2], abs(float(got - 2 * ref)))
        if 2 * ref >= L.P_FLOOR and abs(float(got / (2 * ref) - 1)) > w[0]:
            w[0], w[1] = abs(float(got / (2 * ref) - 1)), t
    return out


def _assert_port_within_bars(port, label, keep=None):
    err = _port_errors(port, keep)
    for df, (rel, t, d) in err.items():
        print(f"{label} df = {df}: worst relative {rel:.3g} at t = {t!r}, worst |d| {d:.3g}")
    rel, df = max((v[0], df) for df, v in err.items())
    d = max(v[2] for v in err.values())
    print(f"{label}: worst relative {rel:.3g} = {rel / L.REL_BAR:.3g} x the bar (df = {df}), worst |d| {d:.3g} = "
          f"{d / L.ABS_BAR:.3g} x the bar, {port.max_iterations} iterations at most")
    assert d <= L.ABS_BAR and rel <= L.REL_BAR, label


def test_port_on_the_dense_grid():
    """The algorithm itself, with the host libm: within the bars over the whole grid, and the continued fraction
    far from its cap of 200 000 iterations (a thread that ran to the cap would stall its wave)."""
    port = Port()
    assert len(_grid()) > 2000
    _assert_port_within_bars(port, "port")
    assert port.max_iterations < 1000


def _a_few(df, t):
    """Three df and, below t = 0.1, every third decade."""
    return df in (1, 21, 262142) and (t >= 0.1 or (t > 0 and round(4 * math.log10(t)) % 12 == 0))


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_bars_catch(name):
    """The mutation table of profiles/cor_t_tail.md, kept true: a port with that one thing wrong misses the bars.
    Without the symmetry swap the continued fraction runs to its cap of 200 000 iterations near x = 1 (t <= 1e-3) and
    is wrong only there, so that row takes a few points of the grid, for time."""
    swap = name == "symmetry swap dropped"
    port = Port(**MUTATIONS[name])
    with pytest.raises(AssertionError):
        _assert_port_within_bars(port, name, _a_few if swap else None)
    assert port.max_iterations == 200000 if swap else port.max_iterations < 1000
