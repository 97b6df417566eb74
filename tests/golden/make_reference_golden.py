"""Writes tests/golden/reference_ici_kt.npz: what the COMPILED reference (oracle/_ref, `make -C oracle ref`) answers on
the designed matrices and degenerate pairs of tests/reference_cases.py.  Data only: the inputs, and per pair x
perspective (x alternative x continuity for the doubles) the reference's four doubles, its twelve counts, its number of
warnings and the reason its warning names.  tests/test_reference_golden.py regenerates it in memory where the compiled
reference is available and asserts equality with the committed file; tests/test_gpu_reference_parity.py reads only
the file.

    python tests/golden/make_reference_golden.py          # needs oracle/_ref or the reference's source tree

Arrays, for each matrix NAME of reference_cases.matrices() and for "deg" (the degenerate pairs, one pair each):
    X_NAME       the matrix, where it is stored (the 46 500-row one is rebuilt by reference_cases and held by
                 sha256_NAME); deg_x / deg_y / deg_len: the degenerate vectors, padded with 0 to the longest
    out_NAME     [P, 2 perspectives, 3 alternatives, 2 continuity, 4] float64, pairs in combn order
    cnt_NAME     [P, 2, 12] int64 in oracle.COUNT_FIELDS order; zeros where the reference returned before its report
    reason_NAME  [P, 2] int8: 0, or 1 (all NA, no warning), 2 / 3 / 4 (told from the warning's text)
    warn_NAME    [P, 2] int8: the number of warnings
    z_NAME       [P, 2, 2 continuity] float64: z_b as the report prints it (six decimals; NaN where there is no report
                 or the variance came out negative), the scale of the p-value's yardstick
The axes follow reference_cases.PERSPECTIVES / ALTERNATIVES / CONTINUITY."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import reference as R  # noqa: E402
from tests import reference_cases as C  # noqa: E402

PATH = os.path.join(HERE, "reference_ici_kt.npz")
KEYS = ("out", "cnt", "reason", "warn", "z")


def _pairs(pairs):
    """pairs: [(x, y)].  The five result arrays."""
    P = len(pairs)
    out = np.empty((P, 2, 3, 2, 4), dtype=np.float64)
    cnt = np.zeros((P, 2, len(C.COUNT_FIELDS)), dtype=np.int64)
    reason = np.zeros((P, 2), dtype=np.int8)
    warn = np.zeros((P, 2), dtype=np.int8)
    z = np.full((P, 2, 2), np.nan)
    for p, (x, y) in enumerate(pairs):
        for s, persp in enumerate(C.PERSPECTIVES):
            seen = set()
            for a, alt in enumerate(C.ALTERNATIVES):
                for c, cont in enumerate(C.CONTINUITY):
                    o, rep, n_warn, rsn, _text = R.ici_kt(x, y, persp, alt, cont)
                    out[p, s, a, c] = o
                    if rep:
                        assert a == 0 or rep["z_b"] == z[p, s, c] or np.isnan(rep["z_b"])
                        z[p, s, c] = rep["z_b"]
                    seen.add((n_warn, rsn, tuple(rep.get(k) for k in R.REPORT_COUNTS)))
            assert len(seen) == 1          # counts, warnings and reason do not depend on alternative or continuity
            warn[p, s], reason[p, s] = n_warn, rsn
            if rep:
                full = R.counts(x, y, persp, report=rep)
                cnt[p, s] = [full[k] for k in C.COUNT_FIELDS]
    return out, cnt, reason, warn, z


def generate():
    arrays = {}
    for m in C.matrices():
        pi, pj = C.pairs_of(m.X.shape[1])
        res = _pairs([(m.X[:, i], m.X[:, j]) for i, j in zip(pi, pj)])
        if m.stored:
            arrays[f"X_{m.name}"] = np.asfortranarray(m.X)
        else:
            arrays[f"sha256_{m.name}"] = np.array(C.digest(m.X))
        for key, a in zip(KEYS, res):
            arrays[f"{key}_{m.name}"] = a
    deg = C.degenerates()
    width = max(len(x) for _n, x, _y in deg)
    arrays["deg_len"] = np.array([len(x) for _n, x, _y in deg], dtype=np.int64)
    for key, col in (("deg_x", 1), ("deg_y", 2)):
        arrays[key] = np.zeros((len(deg), width), dtype=np.float64)
        for k, d in enumerate(deg):
            arrays[key][k, :len(d[col])] = d[col]
    arrays["deg_names"] = np.array([d[0] for d in deg])
    for key, a in zip(KEYS, _pairs([(x, y) for _n, x, y in deg])):
        arrays[f"{key}_deg"] = a
    return arrays


def main():
    np.savez_compressed(PATH, **generate())
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
