"""Which shape of the pre-pass kernel a launch takes (csrc/icikt_k0plan.h: k0_pick_shape, k0_launch_shape), without a
GPU and without the library: tests/k0plan_print.cpp is compiled with the host compiler (with the address and
undefined-behaviour sanitizers where they link) and prints the shape for the (rows, columns) couples on its command
line.  The rule: the large shape whenever the launch has no more columns than the device has CUs; the 512-thread shape
(two columns in flight on a CU) only at the column lengths where the sweep of profiles/k0_two_in_flight.log measured it
faster in every repeat; the debug plan key k0 overrides both.

The same header says how many columns of a host matrix one pre-pass launch covers (k0_chunk_columns: a chunk of
upload_and_prepare); `k0plan_print chunk` prints it for the cases on its standard input, and the expected values are
the parent's (tests/golden/pipeline_parent.json, "chunk_width": recorded once by compiling the expression as it stood
inline in icikt_capi.cpp into a stand-alone program and running it on chunk_cases())."""
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
    run.exe = out
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


# ---- the columns of a chunk of a host matrix (k0_chunk_columns) ----
# tests/golden/pipeline_parent.json, "chunk_width": what the expression gave while it stood inline in upload_and_prepare
# (icikt_capi.cpp) -- those lines were compiled as they were into a stand-alone program and run once on chunk_cases(), in
# that order.  The fixture holds the results only.
PIPE_GOLDEN = os.path.join(ROOT, "tests", "golden", "pipeline_parent.json")
VIEW_COL, VIEW_ROW, VIEW_SPARSE = 0, 1, 2
PREPASS_NONE, PREPASS_FULL, PREPASS_MASK = 0, 1, 2
MB = 1 << 20
# rows of a column: 8 MB hold one (1 048 576 rows), two, three, four, an odd number (107) and an even one (104) of them,
# and many; a half of the staging blocks (64 MB) holds 512-byte runs of a row-major chunk up to 131 072 rows
CHUNK_N_FEAT = (1, 1000, 9799, 10000, 131071, 131072, 131073, 262144, 262145, 349525, 524288, 1048576)
# columns: n_samp / 4 (rounded down to even) on either side of 256 and of 304 CUs
CHUNK_N_SAMP = (2, 301, 1020, 1024, 1028, 1032, 1212, 1216, 1220, 1224, 4096)
CHUNK_VIEWS = ((VIEW_COL, 8), (VIEW_ROW, 4), (VIEW_ROW, 8), (VIEW_SPARSE, 8))
# (prepass, sort_chunk): the sort scratch binds (1, 7, 100 columns; 0 stands for 1) or not; not asked without the full pre-pass
CHUNK_PREPASS = ((PREPASS_FULL, 1 << 20), (PREPASS_FULL, 100), (PREPASS_FULL, 7), (PREPASS_FULL, 1), (PREPASS_FULL, 0),
                 (PREPASS_NONE, 7), (PREPASS_MASK, 7))


def chunk_cases():
    return [(n, S, cus, pipe, view, es, pre, sc) for n in CHUNK_N_FEAT for S in CHUNK_N_SAMP for cus in (256, 304)
            for pipe in (0, 1) for view, es in CHUNK_VIEWS for pre, sc in CHUNK_PREPASS]


@pytest.fixture(scope="module")
def chunk_prog(prog):
    exe = prog.exe

    def run(cases):
        r = subprocess.run([exe, "chunk"], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    return run


def test_chunk_columns_are_the_parent_s(chunk_prog):
    with open(PIPE_GOLDEN) as f:
        want = json.load(f)["chunk_width"]
    cases = chunk_cases()
    got = chunk_prog(cases)
    assert len(got) == len(want) == len(cases)
    for c, g, w in zip(cases, got, want):
        assert g == w, (c, g, w)


def test_chunk_columns_at_the_borders(chunk_prog):
    """Worked by hand from the rule: 8 MB of float64 columns rounded down to an even count, at least two; pipelined: at
    least min(CUs, n_samp / 4 rounded down to even); row-major: at least 512 bytes of cells where 64 MB hold n_feat such
    runs, else what 64 MB hold; the full pre-pass: at most the sort scratch's columns."""
    free = (PREPASS_FULL, 1 << 20)

    def one(n, S=2, cus=256, pipe=0, view=(VIEW_COL, 8), pre=free):
        return chunk_prog([(n, S, cus, pipe, *view, *pre)])[0]
    # 8 MB / column bytes = 1, 2, 3, 4, 107 (odd), 104
    assert [one(n) for n in (1048576, 524288, 349525, 262144, 9799, 10000)] == [2, 2, 2, 4, 106, 104]
    assert one(262145) == 2 and one(1) == 1048576
    # pipelined, 10 000 rows (104 columns): n_samp / 4 below, at and above the CU count
    assert [one(10000, S, 256, 1) for S in (1020, 1024, 1028, 1032, 4096)] == [254, 256, 256, 256, 256]
    assert [one(10000, S, 304, 1) for S in (1212, 1216, 1220, 1224, 4096)] == [302, 304, 304, 304, 304]
    assert one(10000, 301, 256, 1) == 104 and one(10000, 4096, 256, 0) == 104       # 74 columns; not pipelined
    assert one(1000, 1024, 256, 1) == 1048                                          # 8 MB hold more
    # row-major: the 512-byte run of 4- and 8-byte cells, and the 64 MB half on either side of 131 072 rows
    assert [one(n, view=(VIEW_ROW, 8)) for n in (131071, 131072, 131073, 262144)] == [64, 64, 63, 32]
    assert [one(n, view=(VIEW_ROW, 4)) for n in (131071, 131072, 131073, 262144)] == [128, 128, 127, 64]
    assert one(131072, view=(VIEW_COL, 8)) == one(131072, view=(VIEW_SPARSE, 8)) == 8
    assert one(10000, view=(VIEW_ROW, 8)) == 104 and one(10000, 4096, 256, 1, (VIEW_ROW, 4)) == 256
    # the sort scratch binds under the full pre-pass only
    assert [one(10000, pre=(PREPASS_FULL, sc)) for sc in (1 << 20, 104, 100, 7, 1, 0)] == [104, 104, 100, 7, 1, 1]
    assert one(10000, pre=(PREPASS_NONE, 7)) == one(10000, pre=(PREPASS_MASK, 7)) == 104
    assert one(10000, 4096, 256, 1, (VIEW_ROW, 8), (PREPASS_FULL, 7)) == 7


@pytest.mark.parametrize("k0", [LARGE, SMALL, PAIR])
def test_plan_key_overrides(prog, k0):
    couples = [(n, cols) for n in (1, 3000, 10000, 65535) for cols in (1, 96, 256, 257, 1024, 2048)]
    assert prog(k0, CUS, couples)["shape"] == [k0] * len(couples)
    # anything else is the library's choice
    assert prog(7, CUS, couples)["shape"] == prog(-1, CUS, couples)["shape"]
