"""The reference's published answers that both the CPU oracle (tests/test_oracle_golden.py) and the MI355X
(tests/test_gpu_parity.py) must reproduce: inputs and checks shared by the two, numbers from tests/golden/expected.json
(transcribed from the reference's rendered pages; tests/golden/make_golden.py names the lines)."""
import os

import numpy as np
import pytest

from oracle.rrng import RRandom


def check_vignette(res_matrix, res_frame, e):
    """ici_kendalltau(cbind(s1, s2, s3)) in both return forms against the vignette's printed matrix and data frame
    (seven digits, so 5e-8): the only published answer with a taumax below 1 next to one of 1 and a diagonal below 1."""
    tol, names = e["abs_tol"], ["s1", "s2", "s3"]
    cor = res_matrix["cor"].to_numpy()
    assert list(res_matrix["cor"].columns) == names and np.array_equal(cor, cor.T)
    for key, want in e["cor"].items():
        a, b = (names.index(v) for v in key.split("-"))
        assert cor[a, b] == pytest.approx(want, abs=tol), key
    for name, want in e["cor_diag"].items():
        assert cor[names.index(name), names.index(name)] == pytest.approx(want, abs=tol), name
    df = res_frame["cor"]
    for row in e["rows"]:
        got = df[(df["s1"] == row["s1"]) & (df["s2"] == row["s2"])]
        assert len(got) == 1, row
        for k in ("raw", "taumax", "completeness", "cor"):
            if k in row:
                assert float(got[k].iloc[0]) == pytest.approx(row[k], abs=tol), (row["s1"], row["s2"], k)
        a, b = names.index(row["s1"]), names.index(row["s2"])
        for k in ("raw", "taumax", "completeness", "cor"):          # the two forms are one computation
            assert float(got[k].iloc[0]) == pytest.approx(res_matrix[k].to_numpy()[a, b], abs=1e-15), (row, k)


def vignette_matrix(golden_dir):
    z = np.load(os.path.join(golden_dir, "vignette_s1_s3.npz"))
    M = np.column_stack([z["s1"], z["s2"], z["s3"]])
    assert M.shape == (1000, 3) and np.isnan(M).sum(axis=0).tolist() == [0, 0, 15]
    return M


def readme_kt_fast_xy():
    """README.md: x and y are drawn after s1 .. s4 in the same session."""
    rr = RRandom(1234)
    rr.rnorm(1000, 100, 10)
    rr.sample(100, 50)
    rr.sample(100, 50)
    return rr.rnorm(1000), rr.rnorm(1000)


def check_readme_kt_fast(res, e):
    tau, p = res["tau"].to_numpy(), res["pvalue"].to_numpy()
    assert tau[0, 1] == tau[1, 0] == pytest.approx(e["tau"], abs=e["tau_abs_tol"])
    assert p[0, 1] == p[1, 0] == pytest.approx(e["pvalue"], abs=e["pvalue_abs_tol"])
    assert tau[0, 0] == tau[1, 1] == 1.0 and p[0, 0] == p[1, 1] == 0.0


def ici_kt_help_cases(e):
    """(x, y, perspective, expected 4-vector) of the ici_kt help page, for a strictly increasing x that is not R's."""
    x = np.sort(np.random.default_rng(0).normal(size=100))
    assert (np.diff(x) > 0).all()
    y = x + 1
    y2 = y.copy()
    y2[:10] = np.nan
    return [(x, y, "local", e["x_y"]), (x, y2, "global", e["x_y2_global"]), (x, y2, "local", e["x_y2_local"])]


def check_ici_kt_help(out4, want, e):
    assert out4[1] == pytest.approx(want[1], rel=e["pvalue_rel_tol"])
    for k in (0, 2, 3):
        assert out4[k] == pytest.approx(want[k], abs=e["abs_tol"])
