"""The Student-t p-value of ``k_cor_epilogue``, line by line in Python (test infrastructure only).

THIS FILE MIRRORS icikendalltau_amd/csrc/icikt_cor.hip AND HAS TO FOLLOW IT: ``lgammacor``, ``cor_lbeta``,
``incbeta_cf``, ``incbeta``, ``t_tail`` and ``cor_pt`` below are the device functions of those names, statement by
statement and in the device's order of operations, on Python floats (IEEE doubles, the host libm, no contraction).
A change of the device code that is not made here as well makes tests/test_t_tail_exact.py test something the
library no longer runs.

What it is for: the algorithm's own error against tests/t_tail_exact.py on a grid far denser than a device test can
afford, the number of continued-fraction iterations a thread can need, and what the suite's bars catch when the
algorithm is wrong (``Port(...)`` with one of the four mutations).  The device's libm (ocml) and the compiler's
contraction are what it cannot see; tests/test_gpu_cor_t_tail.py runs the device itself on a designed lattice."""
import math


class Port:
    """The six device functions.  The keywords are the mutations of the table in profiles/cor_t_tail.md; the
    defaults are the device's code.  ``iterations`` holds the continued fraction's count of the last call,
    ``max_iterations`` the largest since construction."""

    def __init__(self, stirling_correction=True, eps=1e-16, swap=True, front_scale=1.0):
        self.stirling_correction = stirling_correction
        self.eps = eps
        self.swap = swap
        self.front_scale = front_scale
        self.iterations = 0
        self.max_iterations = 0

    def lgammacor(self, x):
        if not self.stirling_correction:
            return 0.0
        r = 1.0 / x
        r2 = r * r
        return r * (1.0 / 12 + r2 * (-1.0 / 360 + r2 * (1.0 / 1260 + r2 * (-1.0 / 1680 + r2 * (
            1.0 / 1188 + r2 * (-691.0 / 360360))))))

    def cor_lbeta(self, a, b):
        p, q = min(a, b), max(a, b)
        if p >= 10.0:
            corr = self.lgammacor(p) + self.lgammacor(q) - self.lgammacor(p + q)
            return -0.5 * math.log(q) + 0.918938533204672741780329736406 + corr + (p - 0.5) * math.log(p / (p + q)) + \
                q * math.log1p(-p / (p + q))
        if q >= 10.0:
            corr = self.lgammacor(q) - self.lgammacor(p + q)
            return math.lgamma(p) + corr + p - p * math.log(p + q) + (q - 0.5) * math.log1p(-p / (p + q))
        return math.lgamma(p) + math.lgamma(q) - math.lgamma(p + q)

    def incbeta_cf(self, a, b, x, y):
        tiny, eps = 1e-300, self.eps
        front = self.front_scale * math.exp(a * math.log(x) + b * math.log(y) - self.cor_lbeta(a, b)) / a
        f, c, d = 1.0, 1.0, 1.0 - (a + b) * x / (a + 1.0)
        if abs(d) < tiny:
            d = tiny
        d = 1.0 / d
        f = d
        m = 1
        while m < 200000:
            num = m * (b - m) * x / ((a + 2.0 * m - 1.0) * (a + 2.0 * m))
            d = 1.0 + num * d
            if abs(d) < tiny:
                d = tiny
            c = 1.0 + num / c
            if abs(c) < tiny:
                c = tiny
            d = 1.0 / d
            f *= d * c
            num = -(a + m) * (a + b + m) * x / ((a + 2.0 * m) * (a + 2.0 * m + 1.0))
            d = 1.0 + num * d
            if abs(d) < tiny:
                d = tiny
            c = 1.0 + num / c
            if abs(c) < tiny:
                c = tiny
            d = 1.0 / d
            dl = d * c
            f *= dl
            if abs(dl - 1.0) < eps:
                break
            m += 1
        self.iterations = m
        self.max_iterations = max(self.max_iterations, m)
        return front * f

    def incbeta(self, a, b, x, y):
        if x <= 0.0:
            return 0.0
        if y <= 0.0:
            return 1.0
        if self.swap and x > (a + 1.0) / (a + b + 2.0):
            return 1.0 - self.incbeta_cf(b, a, y, x)
        return self.incbeta_cf(a, b, x, y)

    def t_tail(self, t, df):
        if math.isinf(t):
            return 0.0
        t2 = t * t
        return 0.5 * self.incbeta(0.5 * df, 0.5, df / (df + t2), t2 / (df + t2))

    def cor_pt(self, t, df, lower):
        if t != t or not df > 0.0:
            return math.nan
        tail = self.t_tail(t, df)
        return tail if lower == (t < 0.0) else 1.0 - tail


# the mutation table: name -> a port with one thing wrong
MUTATIONS = {
    "lgammacor dropped": dict(stirling_correction=False),
    "eps 1e-6 for 1e-16": dict(eps=1e-6),
    "symmetry swap dropped": dict(swap=False),
    "front halved": dict(front_scale=0.5),
}
