"""Which shape of the pre-pass kernel a launch takes (csrc/icikt_k0plan.h: k0_pick_shape, k0_launch_shape), without a
GPU and without the library: tests/k0plan_print.cpp is compiled with the host compiler (with the address and
undefined-behaviour sanitizers where they link) and prints the shape for the (rows, columns) couples on its command
line.  The rule: the large shape whenever the launch has no more columns than the device has CUs; the 512-thread shape
(two columns in flight on a CU) only at the column lengths where the sweep of profiles/k0_two_in_flight.log measured it
faster in every repeat; the debug plan key k0 overrides both."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "k0plan_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")

LARGE, SMALL, PAIR = 0, 1, 2
# the measured range (profiles/k0_two_in_flight.log, section 3): rows of a column, both ends included
PAIR_ROWS = (300, 10000)
PAIR_MIN_COLUMNS_PER_CU = 2                # the narrowest launches the sweep has (512 columns on 256 CUs)
SWEPT_ROWS = (300, 1000, 2000, 3000, 4096, 4097, 6000, 8192, 8193, 10000, 12000, 12288, 14000, 16000, 16384, 16385, 18000,
              20000, 50000)
CUS = 256                              # an MI355X


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("k0plan") / "k0plan_print")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:   # (no sanitizer runtime here)
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr

    def run(k0, cus, couples):
        args = [str(int(x)) for c in couples for x in c]
        r = subprocess.run([out, str(k0), str(cus), *args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    return run


def test_constants(prog):
    got = prog(-1, CUS, [])
    assert (got["large"], got["small"], got["pair"]) == (LARGE, SMALL, PAIR)
    assert (got["min_rows"], got["max_rows"]) == PAIR_ROWS
    assert got["min_columns_per_cu"] == PAIR_MIN_COLUMNS_PER_CU
    assert got["shape"] == []


def test_large_shape_when_the_launch_has_no_columns_to_spare(prog):
    """c3 (256 columns), c2 (96) and the chunks of multi-GPU shards: a single round of workgroups either way."""
    ns = (1, 64, 3000, 6887, 10000, 20000, 50000, 65535)
    for cus in (1, 104, 256, 304):
        couples = [(n, cols) for n in ns for cols in sorted({0, 1, cus // 2, cus - 1, cus})]
        assert prog(-1, cus, couples)["shape"] == [LARGE] * len(couples), cus
    # the benchmark's configurations on an MI355X
    assert prog(-1, CUS, [(10000, 256), (6887, 96)])["shape"] == [LARGE, LARGE]


def test_pair_shape_only_inside_the_measured_range(prog):
    lo, hi = PAIR_ROWS
    ns = sorted(set([1, 2, 63, 64, 65, 1000, 4096, 4097, 8192, 8193, 12288, 16384, 16385, 30000, 65535, 65536, 70000, 262144,
                     *SWEPT_ROWS, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1]))
    ns = [n for n in ns if n >= 0]
    for cols in (2 * CUS, 2 * CUS + 1, 1024, 2048, 100000):
        got = prog(-1, CUS, [(n, cols) for n in ns])["shape"]
        want = [PAIR if lo <= n <= hi else LARGE for n in ns]
        assert got == want, cols
    assert PAIR in prog(-1, CUS, [(n, 2 * CUS) for n in ns])["shape"]
    # more columns than CUs, fewer than two per CU: the sweep has no such launch, the large shape stays
    for cols in (CUS + 1, CUS + CUS // 2, 2 * CUS - 1):
        assert prog(-1, CUS, [(n, cols) for n in ns])["shape"] == [LARGE] * len(ns), cols
    # the rule counts in CUs of the device at hand
    assert prog(-1, 304, [(10000, 607), (10000, 608)])["shape"] == [LARGE, PAIR]
    assert set(prog(-1, CUS, [(n, 1024) for n in ns])["shape"]) <= {LARGE, PAIR}   # the small shape is never the library's choice
    # no device (no CU count): the large shape
    assert prog(-1, 0, [(10000, 1024)])["shape"] == [LARGE]


def test_c4_takes_what_was_measured(prog):
    """The flagship step: 10 000 rows x 1 024 columns."""
    assert prog(-1, CUS, [(10000, 1024)])["shape"] == [PAIR]


@pytest.mark.parametrize("k0", [LARGE, SMALL, PAIR])
def test_plan_key_overrides(prog, k0):
    couples = [(n, cols) for n in (1, 3000, 10000, 65535) for cols in (1, 96, 256, 257, 1024, 2048)]
    assert prog(k0, CUS, couples)["shape"] == [k0] * len(couples)
    # anything else is the library's choice
    assert prog(7, CUS, couples)["shape"] == prog(-1, CUS, couples)["shape"]
