"""Student's t tail at 400 digits (test infrastructure only): the yardstick of the t branch of cor_fast's p-values.

``t_tail_exact(rho, df)`` is P(T > |t|) for t = sqrt(df) rho / sqrt(1 - rho^2), taken directly from the double rho:
x = 1 - rho^2 and y = rho^2 are formed exactly (as fractions) and never pass through a double t or a double x, so the
roundings the library makes on the way from rho to the incomplete beta function are part of what a comparison tests.
``t_tail_exact_t(t, df)`` is the same from a double t (x = df / (df + t^2), y = t^2 / (df + t^2), exactly).

Both use one formula, the series with positive terms only

    I_z(p, q) = z^p (1 - z)^q / (p B(p, q)) * sum_k (p + q)_k / (p + 1)_k z^k,        0 <= z <= 1/2,

as  tail = I_x(df/2, 1/2) / 2  when x <= 1/2  and  tail = (1 - I_y(1/2, df/2)) / 2  otherwise.  The one subtraction,
in the complement, loses as many digits as the tail has leading zeros: 400 digits cover every tail >= 1e-300 with 80
to spare.  B(p, q) comes from mpmath.loggamma.  No continued fraction, no symmetry swap at (a + 1) / (a + b + 2), no
Stirling correction, no scipy: nothing here shares code or a method with icikt_cor.hip or with api._t_tail.
tests/test_t_tail_exact.py holds it to the closed forms at df = 1, 2 and to scipy.stats.t.sf."""
import functools
from fractions import Fraction

import mpmath

DPS = 400
_WORK = DPS + 30                          # guard digits for the products and the truncations of the series
_PREC = int(_WORK * 3.3219280948873626) + 1
ALTERNATIVES = ("two.sided", "less", "greater")


@functools.lru_cache(maxsize=None)
def _log_beta_half(df):
    """log B(df/2, 1/2)."""
    with mpmath.workdps(_WORK):
        a, b = mpmath.mpf(df) / 2, mpmath.mpf(1) / 2
        return mpmath.loggamma(a) + mpmath.loggamma(b) - mpmath.loggamma(a + b)


def _mpf(fr):
    return mpmath.mpf(fr.numerator) / mpmath.mpf(fr.denominator)


def _series(z, p2, q2):
    """sum_k (p + q)_k / (p + 1)_k z^k for p = p2/2, q = q2/2 (p2, q2 positive integers) and 0 < z <= 1/2, in fixed
    point with _PREC fraction bits.  The terms rise from 1 to a peak near k = q z / (1 - z) and then fall, at last by
    the factor z per step, so the first term that truncates to 0 ends the sum; every truncation loses less than
    2^-_PREC of a sum that is at least 1."""
    zf = int(mpmath.floor(mpmath.ldexp(z, _PREC)))
    term = total = 1 << _PREC
    num, den = p2 + q2, p2 + 2
    while term:
        term = ((term * zf) >> _PREC) * num // den
        total += term
        num += 2
        den += 2
    return mpmath.ldexp(mpmath.mpf(total), -_PREC)


def _inc_beta(z, w, p2, q2, df):
    """I_z(p2/2, q2/2) with w = 1 - z, for 0 < z <= 1/2; {p2, q2} = {df, 1}."""
    p, q = mpmath.mpf(p2) / 2, mpmath.mpf(q2) / 2
    front = mpmath.exp(p * mpmath.log(z) + q * mpmath.log(w) - _log_beta_half(df)) / p
    return front * _series(z, p2, q2)


def _tail_xy(x, y, df):
    """P(T > |t|) from the exact fractions x = df / (df + t^2) and y = 1 - x."""
    if int(df) != df or df < 1:
        raise ValueError("df must be a positive integer")
    df = int(df)
    with mpmath.workdps(_WORK):
        if y == 0:
            return mpmath.mpf(1) / 2
        if x == 0:
            return mpmath.mpf(0)
        xm, ym = _mpf(x), _mpf(y)
        if 2 * x <= 1:
            return _inc_beta(xm, ym, df, 1, df) / 2
        return (1 - _inc_beta(ym, xm, 1, df, df)) / 2


@functools.lru_cache(maxsize=1 << 16)
def t_tail_exact(rho, df):
    """P(T > |t|), t = sqrt(df) rho / sqrt(1 - rho^2), for the double rho in [-1, 1]; an mpmath.mpf."""
    r = Fraction(float(rho))
    if abs(r) > 1:
        raise ValueError("rho outside [-1, 1]")
    return _tail_xy(1 - r * r, r * r, df)


@functools.lru_cache(maxsize=1 << 16)
def t_tail_exact_t(t, df):
    """P(T > |t|) for the finite double t; an mpmath.mpf."""
    t2 = Fraction(float(t)) ** 2
    return _tail_xy(Fraction(int(df)) / (int(df) + t2), t2 / (int(df) + t2), df)


def t_pvalue_exact(rho, df, alternative="two.sided"):
    """cor.test's p-value from the t distribution at the estimate rho: twice the tail, or pt(t, df) ("less") /
    1 - pt(t, df) ("greater"), of which one is the tail and the other its complement; an mpmath.mpf."""
    if alternative not in ALTERNATIVES:
        raise ValueError(alternative)
    tail = t_tail_exact(rho, df)
    with mpmath.workdps(_WORK):
        if alternative == "two.sided":
            return 2 * tail
        return tail if (alternative == "less") == (rho < 0) else 1 - tail


def on_tail_side(rho, alternative):
    """Whether t_pvalue_exact(rho, df, alternative) is the tail itself (or twice it), not a complement."""
    return alternative == "two.sided" or (alternative == "less") == (rho < 0)
