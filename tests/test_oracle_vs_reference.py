"""The CPU oracle (oracle/icikt_oracle.c, a transcription) against the COMPILED reference: the reference's own
src/kendallc.cpp built against oracle/rcpp_standin/Rcpp.h (`make -C oracle ref`, oracle/reference.py).

On a designed lattice -- n = 2 ... 3 000 with ties, scattered and shared NaN, both perspectives, the three alternatives,
continuity; the fixture matrices of tests/reference_cases.py with their tie groups of 1 100, 1 300 and 46 400 rows and
one of 2 500; the degenerate pairs; the pairs of the committed vector fixtures -- it asserts:
  doubles    tau, tau_max and completeness bit for bit (a difference is a finding, not a tolerance);
  counts     all twelve fields exact: eight from the reference's report, the six tie sums from the reference's own
             sortedIndex / compare_self / cumsum / count_rank_tie on the filled columns, dis once more from its
             kendall_discordant;
  p-value    the scaled error of tests/epilogue_checker.py at the CPU bar, 2 E_CPU (Cody's pnorm in the oracle against
             erfcl in the stand-in, which is the better-rounded side); the worst is printed (-s) and recorded in
             profiles/epilogue_tails.md;
  NA         the pattern field by field, R's payload, reason != 0 exactly when the reference returns all NA, reasons
             2 / 3 / 4 exactly when it warned once (and the warning is that reason's), reason 1 without a warning;
  variants   the plain build and the -fwrapv build agree in every bit and every character of the report;
  control    the oracle with int32_compat=False DIFFERS from the reference on every pair in the int32 regime and on no
             other: the lattice sits in the regime and the comparison can fail.
Skips only where neither oracle/_ref nor the reference's source tree exists."""
import collections
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import reference as R
from tests import epilogue_checker as E
from tests import reference_cases as C

pytestmark = pytest.mark.skipif(not R.available(), reason="no compiled reference and no reference tree to build it from")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NA_BITS = np.uint64(0x7FF00000000007A2)
SETTINGS = [(a, c) for a in C.ALTERNATIVES for c in C.CONTINUITY]
P_BOUND = 2 * E.E_CPU["cases"]

Pair = collections.namedtuple("Pair", "group name x y settings")
Record = collections.namedtuple("Record", "pair perspective alternative continuity o ocnt oreason r rep nwarn rreason text")


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _lattice():
    """n x 6 variants: continuous / tied x, tied y, NaN scattered over each column by its own modulus, and (variant 5)
    a fifth of the rows missing in BOTH."""
    out = []
    for n in (2, 3, 5, 64, 65, 300, 1500, 3000):
        p = {2: 3, 3: 5, 5: 7, 64: 67, 65: 67, 300: 307, 1500: 1511, 3000: 3001}[n]
        for v in range(6):
            a, b = 1 + (p * (3 + v)) // 11 % (p - 1), 1 + (p * (5 + 2 * v)) // 13 % (p - 1)
            x = (C.scatter(n, a, p) - p // 2).astype(np.float64) / 8.0
            y = (C.scatter(n, b, p) + (v - 3) * C.scatter(n, a, p) // 4).astype(np.float64) / 4.0
            if v % 2:
                x = np.round(x / (1, 3, 20)[v // 2])
            if v % 3 == 0:
                y = np.round(y / (5, 40)[v // 3])
            if n > 3:
                x[C.scatter(n, b, p, 1) % 7 == 0] = np.nan
                y[C.scatter(n, a, p, 2) % 6 == 0] = np.nan
            if v == 5:
                both = C.scatter(n, a, p, 3) % 5 == 0
                x[both] = np.nan
                y[both] = np.nan
            out.append(Pair("lattice", f"n{n}v{v}", x, y, SETTINGS))
    return out


def _matrix_pairs(group, name, X, settings, cols=None):
    cols = range(X.shape[1]) if cols is None else cols
    return [Pair(group, f"{name}[{i},{j}]", X[:, i], X[:, j], settings) for k, i in enumerate(cols) for j in list(cols)[k + 1:]]


def _g2500():
    n, g = 4000, 2500
    X = np.empty((n, 3))
    X[:, 0] = C.scatter(n, 1777, 4001) / 8.0
    rows = C.shuffle(n, 911, 4001)
    X[rows[:g], 0] = 0.5
    X[:, 1] = C.scatter(n, 2311, 4003) / 4.0
    X[rows[g // 2:g // 2 + g], 1] = np.nan
    X[:, 2] = (C.scatter(n, 3301, 4007) % 5).astype(np.float64)
    return X


def _golden():
    out = []
    for f in ("readme_s1_s4.npz", "vignette_s1_s3.npz", "snapshot_50000.npz"):       # the fixtures that hold vectors
        z = np.load(os.path.join(GOLDEN, f))
        names = sorted(z.files)
        out += [Pair("golden", f"{f}:{a},{b}", z[a], z[b], SETTINGS) for k, a in enumerate(names) for b in names[k + 1:]]
    plain = [("two.sided", False)]
    for f, cols in (("ktfast_100x4.npz", None), ("completeness_50x100.npz", range(0, 100, 7)),
                    ("include_only_50x100.npz", range(0, 100, 7)), ("missing_dataset.npz", None),
                    ("yeast_missing.npz", range(0, 96, 12))):
        out += _matrix_pairs("golden", f, np.load(os.path.join(GOLDEN, f))["X"], plain, cols)
    return out


def all_pairs():
    out = _lattice()
    for m in C.matrices():
        out += _matrix_pairs("wrap" if m.wraps else "lattice", m.name, m.X, SETTINGS if m.name != "xtie" else SETTINGS[:2])
    out += _matrix_pairs("wrap", "g2500", _g2500(), SETTINGS[:1])
    out += [Pair("degenerate", name, x, y, SETTINGS) for name, x, y in C.degenerates()]
    return out + _golden()


@pytest.fixture(scope="module")
def records():
    recs = []
    for pair in all_pairs():
        for persp in C.PERSPECTIVES:
            for alt, cont in pair.settings:
                o, ocnt, oreason = O.ici_kt(pair.x, pair.y, persp, alt, cont)
                r, rep, nwarn, rreason, text = R.ici_kt(pair.x, pair.y, persp, alt, cont)
                recs.append(Record(pair, persp, alt, cont, o, ocnt, oreason, r, rep, nwarn, rreason, text))
    return recs


def _where(rec):
    return f"{rec.pair.group}/{rec.pair.name} {rec.perspective} {rec.alternative} continuity={rec.continuity}"


def test_the_lattice_is_the_one_described(records):
    groups = collections.Counter(rec.pair.group for rec in records)
    assert len(records) >= 605 and groups["lattice"] >= 576 and groups["wrap"] >= 24 and groups["degenerate"] >= 5
    assert groups["golden"] >= 10 * 12
    ok = [rec for rec in records if rec.rreason == 0]
    assert len(ok) > 0.8 * len(records)
    assert {rec.rreason for rec in records} == {0, 1, 2, 3}          # (4 has no input: tests/reference_cases.py)
    assert sum(rec.perspective == "local" and rec.ocnt["n"] < len(rec.pair.x) for rec in ok) > 100   # local != global


def test_tau_taumax_completeness_bit_for_bit(records):
    bad = [(_where(rec), k, float(rec.o[k]), float(rec.r[k])) for rec in records for k in (0, 2, 3)
           if bits(rec.o)[k] != bits(rec.r)[k]]
    assert not bad, (len(bad), bad[:5])


def test_na_pattern_reasons_and_warnings(records):
    bad = []
    for rec in records:
        o, r = rec.o, rec.r
        if not np.array_equal(np.isnan(o), np.isnan(r)):
            bad.append((_where(rec), "pattern", o, r))
        if (rec.oreason != 0) != bool(np.isnan(r).all()):
            bad.append((_where(rec), "reason without all-NA", rec.oreason, r))
        if np.isnan(r).all() and not (np.all(bits(r) == NA_BITS) and np.all(bits(o) == NA_BITS)):
            bad.append((_where(rec), "payload", bits(o), bits(r)))
        if (rec.oreason in (2, 3, 4)) != (rec.nwarn == 1) or rec.nwarn > 1 or (rec.oreason == 1 and rec.nwarn):
            bad.append((_where(rec), "warnings", rec.oreason, rec.nwarn))
        if rec.oreason != rec.rreason:
            bad.append((_where(rec), "reason", rec.oreason, rec.rreason))
        if bool(rec.rep) != (rec.rreason == 0):                       # the report is printed exactly when there is a result
            bad.append((_where(rec), "report", rec.rreason))
    assert not bad, (len(bad), bad[:5])


def test_all_twelve_counts(records):
    """Once per pair and perspective (the counts do not depend on the alternative or on continuity: asserted)."""
    seen = {}
    bad = []
    for rec in records:
        if rec.rreason != 0:
            continue
        key = (rec.pair.group, rec.pair.name, rec.perspective)
        if key not in seen:
            seen[key] = R.counts(rec.pair.x, rec.pair.y, rec.perspective, report=rec.rep)
            assert set(seen[key]) == set(O.COUNT_FIELDS)
        want = seen[key]
        assert all(rec.rep[label] == want[field] for label, field in R.REPORT_COUNTS.items()), _where(rec)
        if rec.ocnt != want:
            bad.append((_where(rec), {k: (rec.ocnt[k], want[k]) for k in want if rec.ocnt[k] != want[k]}))
    assert len(seen) > 300 and not bad, (len(bad), bad[:5])


def test_p_value_at_the_cpu_bar(records):
    worst, at = 0.0, None
    worst_rel = 0.0
    bad = []
    for rec in records:
        if rec.rreason != 0:
            continue
        po, pr, z = float(rec.o[1]), float(rec.r[1]), rec.rep["z_b"]
        if np.isnan(pr) or np.isnan(po):                              # sqrt of a wrapped, negative variance
            if not (np.isnan(pr) and np.isnan(po)):
                bad.append((_where(rec), po, pr))
        elif pr == 0.0 or pr == 1.0 and abs(z) >= E.CUTOFF:
            if po != pr:
                bad.append((_where(rec), po, pr))
        elif pr >= E.TINY:
            e = E.scaled_error(po, pr, z)
            worst_rel = max(worst_rel, abs(po - pr) / pr)
            if e > worst:
                worst, at = e, (_where(rec), z, po, pr)
            if not e <= P_BOUND:
                bad.append((_where(rec), po, pr, e))
        elif not abs(po - pr) <= P_BOUND * (1 + z * z) * E.UNIT * pr + 4 * 2.0 ** -1074:
            bad.append((_where(rec), po, pr))
    print(f"\noracle against the compiled reference: worst scaled p error {worst:.3f} (bar {P_BOUND}) at {at}; "
          f"worst relative difference {worst_rel:.3g}")
    assert not bad, (len(bad), bad[:5])


def test_plain_and_wrapv_builds_agree(records):
    seen = set()
    n = 0
    for rec in records:
        r2, _rep2, nwarn2, reason2, text2 = R.ici_kt(rec.pair.x, rec.pair.y, rec.perspective, rec.alternative,
                                                     rec.continuity, variant="wrapv")
        assert np.array_equal(bits(rec.r), bits(r2)) and text2 == rec.text and \
            (nwarn2, reason2) == (rec.nwarn, rec.rreason), _where(rec)
        key = (rec.pair.group, rec.pair.name, rec.perspective)
        if rec.rreason == 0 and key not in seen and (rec.pair.group == "wrap" or len(seen) % 9 == 0):
            assert R.counts(rec.pair.x, rec.pair.y, rec.perspective, "wrapv") == \
                R.counts(rec.pair.x, rec.pair.y, rec.perspective, report=rec.rep), _where(rec)
            n += 1
        seen.add(key)
    assert n > 50


def test_negative_control_exact_sums_differ_exactly_in_the_int32_regime(records):
    """int32_compat=False is the other reading of kendallc.cpp:112-114 and :267.  It must disagree with the compiled
    reference (counts or doubles) on every pair whose exact sums leave int32 -- told from the group sizes in Python
    integers, not from either program -- and agree bit for bit on every other."""
    regime = {}
    n_wrap = 0
    bad = []
    for rec in records:
        if rec.rreason != 0:
            continue
        key = (rec.pair.group, rec.pair.name, rec.perspective)
        if key not in regime:
            regime[key] = C.in_int32_regime(rec.pair.x, rec.pair.y, rec.perspective)
        o, ocnt, oreason = O.ici_kt(rec.pair.x, rec.pair.y, rec.perspective, rec.alternative, rec.continuity,
                                    int32_compat=False)
        same_counts = all(ocnt[field] == rec.rep[label] for label, field in R.REPORT_COUNTS.items()) and \
            all(ocnt[k] == rec.ocnt[k] for k in ("x0", "x1", "y0", "y1"))       # (rec.ocnt equals the reference's: above)
        same = oreason == 0 and same_counts and all(bits(o)[k] == bits(rec.r)[k] for k in (0, 2, 3)) and \
            (o[1] == rec.o[1] or (np.isnan(o[1]) and np.isnan(rec.o[1])))
        n_wrap += regime[key]
        if same == regime[key]:
            bad.append((_where(rec), "in the regime" if regime[key] else "outside it", "same" if same else "differs"))
    in_regime = {k for k, v in regime.items() if v}
    assert not bad, (len(bad), bad[:5])
    groups = {k[0] for k in in_regime}                                # (a golden matrix with many missing rows may be in it)
    assert n_wrap >= 24 and "wrap" in groups and not groups & {"lattice", "degenerate"}, sorted(in_regime)[:10]
    for name in ("t1", "t0", "xtie", "g2500"):                        # every wrap matrix reaches the regime
        assert any(k[1].startswith(name + "[") for k in in_regime), name
    assert any(not v for k, v in regime.items() if k[0] == "wrap")     # ... and has pairs outside it
