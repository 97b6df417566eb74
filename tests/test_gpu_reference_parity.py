"""The HIP engine against the COMPILED reference, through the committed fixture tests/golden/reference_ici_kt.npz (what
the reference's own src/kendallc.cpp answered, tests/golden/make_reference_golden.py) -- not through the CPU oracle,
which is a transcription.  It reads the fixture and tests/reference_cases.py (which rebuilds the 46 500-row matrix and
checks its digest) and nothing of the reference, so it never skips.

Every block -- step (n = 65), t1 (1 500 rows, a group of 1 100: x1 wraps), t0 (1 700, a group of 1 300: the truncating
t0 / 2 of a wrapped sum), xtie (46 500, a group of 46 400: xtie negative, ntie wrapped; whole-wave kernels) and the
degenerate pairs -- goes through three routes, Context.pairs (all pairs with counts), Context.pair and api.ici_kt, for
every perspective x alternative x continuity:
  counts, reasons, NA   the counts the device returns (eleven; the twelfth, sum_obs, through the report api.ici_kt
                        prints), the reason and the NA pattern exact, R's NA payload, a warning exactly where the
                        reference warned;
  doubles               tau, tau_max, completeness within ATOL = 1e-10;
  p-value               the scaled error of tests/epilogue_checker.py at the device bar, 4 E_CPU, with the reference's
                        own z; exactly 0 or 1 beyond the cut-off;
  exact mode            with ICIKT_FLAG_EXACT_INT64 the counts differ from the fixture on exactly the pairs whose exact
                        sums leave int32 (told from the group sizes in Python integers)."""
import warnings

import numpy as np
import pytest

from tests import epilogue_checker as E
from tests import reference_cases as C

pytestmark = pytest.mark.gpu

ATOL = 1e-10                                     # BASELINE.json north_star: the four doubles
P_BOUND = 4 * E.E_CPU["cases"]                   # the device bar (tests/test_gpu_epilogue_tails.py says why 4)
NA_BITS = np.uint64(0x7FF00000000007A2)
BLOCKS = C.MATRIX_NAMES + ("deg",)
SETTINGS = [(s, a, c) for s in range(2) for a in range(3) for c in range(2)]
N_DEVICE_COUNTS = 11                             # _lib.CNT_FIELDS: COUNT_FIELDS without sum_obs


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fx():
    return C.load_fixture()


def _block(fx, name):
    """[(pair index, X of that pair's call, i, j)]: a matrix block is one X for all its pairs, a degenerate pair has
    its own two-column X."""
    if name == "deg":
        return [(k, np.asfortranarray(np.stack([x, y], axis=1)), 0, 1) for k, (_n, x, y) in enumerate(C.fixture_degenerates(fx))]
    X = C.fixture_matrix(fx, name)
    return [(k, X, int(i), int(j)) for k, (i, j) in enumerate(zip(*C.pairs_of(X.shape[1])))]


class Worst:
    def __init__(self):
        self.d, self.p, self.n, self.n_ok = 0.0, 0.0, 0, 0

    def __str__(self):
        return (f"{self.n} results ({self.n_ok} with a value): worst |d| of tau / tau_max / completeness {self.d:.3g} "
                f"(bar {ATOL}), worst scaled p error {self.p:.3f} (bar {P_BOUND})")


def _check(fx, name, k, s, a, c, out, cnt, reason, worst, counts_equal=True):
    """One result (out [4], cnt: the device's eleven counts or None, reason) against the fixture's [k, s, a, c]."""
    where = (name, k, C.PERSPECTIVES[s], C.ALTERNATIVES[a], C.CONTINUITY[c])
    want = fx[f"out_{name}"][k, s, a, c]
    out = np.asarray(out, dtype=np.float64)
    worst.n += 1
    assert int(reason) == int(fx[f"reason_{name}"][k, s]), where
    assert np.array_equal(np.isnan(out), np.isnan(want)), (where, out, want)
    if reason:
        assert np.all(bits(out) == NA_BITS) and np.all(bits(want) == NA_BITS), (where, out)
        return
    worst.n_ok += 1
    if cnt is not None and counts_equal:
        assert [int(v) for v in cnt[:N_DEVICE_COUNTS]] == fx[f"cnt_{name}"][k, s, :N_DEVICE_COUNTS].tolist(), where
    d = float(np.max(np.abs(out[[0, 2, 3]] - want[[0, 2, 3]])))
    worst.d = max(worst.d, d)
    assert d <= ATOL, (where, out, want)
    p, pw, z = float(out[1]), float(want[1]), float(fx[f"z_{name}"][k, s, c])
    if np.isnan(pw):
        return
    if abs(z) >= E.CUTOFF + 1e-5:                 # (z is the report's, six decimals)
        assert pw in (0.0, 1.0) and p == pw, (where, p, pw)
    elif pw >= E.TINY:
        e = E.scaled_error(p, pw, z)
        worst.p = max(worst.p, e)
        assert e <= P_BOUND, (where, p, pw, z, e)
    else:
        assert abs(p - pw) <= P_BOUND * (1 + z * z) * E.UNIT * pw + 4 * 2.0 ** -1074, (where, p, pw)


@pytest.mark.parametrize("name", BLOCKS)
def test_pairs_route(hip_ctx, fx, name):
    worst = Worst()
    block = _block(fx, name)
    calls = [(block[0][1], None, None, [k for k, *_ in block])] if name != "deg" else \
        [(X, np.array([i], np.int32), np.array([j], np.int32), [k]) for k, X, i, j in block]
    for X, pi, pj, ks in calls:
        for s, a, c in SETTINGS:
            out, cnt, rsn = hip_ctx.pairs(X, pi, pj, C.PERSPECTIVES[s], C.ALTERNATIVES[a], C.CONTINUITY[c])
            assert out.shape == (len(ks), 4) and cnt.shape == (len(ks), N_DEVICE_COUNTS)
            for row, k in enumerate(ks):
                _check(fx, name, k, s, a, c, out[row], cnt[row], rsn[row], worst)
    print(f"\nContext.pairs {name}: {worst}")
    assert worst.n == len(block) * len(SETTINGS)


@pytest.mark.parametrize("name", BLOCKS)
def test_pair_route(hip_ctx, fx, name):
    worst = Worst()
    for k, X, i, j in _block(fx, name):
        x, y = np.ascontiguousarray(X[:, i]), np.ascontiguousarray(X[:, j])
        for s, a, c in SETTINGS:
            out, cnt, rsn = hip_ctx.pair(x, y, C.PERSPECTIVES[s], C.ALTERNATIVES[a], C.CONTINUITY[c])
            _check(fx, name, k, s, a, c, out, [cnt[f] for f in C.COUNT_FIELDS[:N_DEVICE_COUNTS]], rsn, worst)
    print(f"\nContext.pair {name}: {worst}")


@pytest.mark.parametrize("name", BLOCKS)
def test_api_route(fx, name, capsys):
    """api.ici_kt: the four doubles of every setting, a RuntimeWarning exactly where the reference warned (reasons 2, 3:
    one warning; reason 1 and results: none), and once per pair and perspective the report it prints for
    output != "simple": the eight integer lines equal the reference's, sum_obs among them, and no report where the
    reference returned before its own."""
    from icikendalltau_amd import api
    from oracle.reference import REPORT_COUNTS, parse_report          # (pure Python: the labels and the line parser)
    worst = Worst()
    for k, X, i, j in _block(fx, name):
        x, y = X[:, i], X[:, j]
        for s, a, c in SETTINGS:
            reason = int(fx[f"reason_{name}"][k, s])
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                res = api.ici_kt(x, y, C.PERSPECTIVES[s], C.ALTERNATIVES[a], C.CONTINUITY[c])
            assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == int(fx[f"warn_{name}"][k, s]), \
                (name, k, s, reason)
            _check(fx, name, k, s, a, c, np.array(tuple(res)), None, reason, worst)
        for s in range(2):
            capsys.readouterr()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                api.ici_kt(x, y, C.PERSPECTIVES[s], output="report")
            rep = parse_report(capsys.readouterr().out)
            if fx[f"reason_{name}"][k, s]:
                assert rep == {}, (name, k, s, rep)
            else:
                want = dict(zip(C.COUNT_FIELDS, fx[f"cnt_{name}"][k, s].tolist()))
                assert {f: rep[label] for label, f in REPORT_COUNTS.items()} == {f: want[f] for f in REPORT_COUNTS.values()}, \
                    (name, k, s)
    print(f"\napi.ici_kt {name}: {worst}")


@pytest.mark.parametrize("name", BLOCKS)
def test_exact_mode_differs_exactly_on_the_wrap_pairs(hip_ctx, fx, name):
    """ICIKT_FLAG_EXACT_INT64: the counts equal the fixture's where every exact sum fits int32 and differ where one
    does not -- the regime told from the group sizes, not from either program -- and the exact counts are the sums in
    Python integers.  t1 and t0 have pairs on both sides of the line."""
    from icikendalltau_amd import _lib
    block = _block(fx, name)
    n_in = n_out = 0
    for s, persp in enumerate(C.PERSPECTIVES):
        calls = [(block[0][1], None, None, block)] if name != "deg" else \
            [(X, np.array([i], np.int32), np.array([j], np.int32), [(k, X, i, j)]) for k, X, i, j in block]
        for X, pi, pj, rows in calls:
            out, cnt, rsn = hip_ctx.pairs(X, pi, pj, persp, flags=_lib.FLAG_EXACT_INT64)
            for row, (k, _X, i, j) in enumerate(rows):
                assert int(rsn[row]) == int(fx[f"reason_{name}"][k, s]), (name, k, persp)
                if rsn[row]:
                    continue
                want = fx[f"cnt_{name}"][k, s, :N_DEVICE_COUNTS]
                regime = C.in_int32_regime(X[:, i], X[:, j], persp)
                assert np.array_equal(cnt[row], want) != regime, (name, k, persp, regime, cnt[row], want)
                x2, y2 = C.fill(X[:, i], X[:, j], persp)
                xs, ys = C.exact_tie_sums(x2), C.exact_tie_sums(y2)
                got = dict(zip(C.COUNT_FIELDS, (int(v) for v in cnt[row])))
                assert (got["xtie"], got["x0"], got["x1"], got["ytie"], got["y0"], got["y1"], got["ntie"]) == \
                    (*xs, *ys, C.exact_joint_ties(x2, y2)), (name, k, persp)
                assert all(got[f] == int(want[C.COUNT_FIELDS.index(f)]) for f in ("n", "missing", "dis", "tot"))
                n_in += regime
                n_out += not regime
    print(f"\nexact mode {name}: {n_in} pair x perspective in the int32 regime, {n_out} outside")
    assert (n_in > 0) == C.matrix(name).wraps if name != "deg" else n_in == 0
    assert n_out > 0 or name == "xtie"           # (each of its three pairs holds a column with a 46 400-row group)
