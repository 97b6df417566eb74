"""The pair kernel's launch plan, tie verdict, task list and grid (csrc/icikt_k1plan.h: plan_k1, tie_verdict,
combn_pairs, build_units, k1_grid), without a GPU and without the library: tests/k1plan_print.cpp is compiled with the
host compiler (with the address and undefined-behaviour sanitizers where they link), reads cases on its standard input
and prints one JSON value per case.

What it must print is tests/golden/k1plan_parent.json: the answers of the code as it stood in icikt_capi.cpp before the
move into the header, recorded once by running that code on the cases below.  The fixture holds results only -- the
cases are generated here, in a fixed order:
  plan_rows    the K1Plan fields [np, wpb, lds_bytes, perpair_bytes, opts, half_items, stride, split] of every case of
               the plan grid without an override on 256 CUs;
  plan_sha256  per (plan key, CUs) the SHA-256 of the printed rows of the whole grid;
  tied, combn, units, grid   the printed values of the other cases, in full.
Beside equality with the fixture the tests assert what must hold whatever the plan decides: the LDS a plan asks for,
the task list's invariants, the verdict on either side of its thresholds and the grid's arithmetic.

The task slices of the pipelined host entries (combn_chunk_units, order_units_by_chunk: the tasks by the chunk in which
their last column arrives) have their cases and their fixture, tests/golden/pipeline_parent.json, at the end of the
file; how that fixture was recorded is said there."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "k1plan_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "k1plan_parent.json")

# ---- the plan grid ----
# rows of a column: every value at which a branch of plan_k1 can flip
NS = (1, 64, 2047, 2048, 8137, 10176, 10177, 12224, 12225, 14272, 14273, 15199, 15200, 16320, 16321, 18336, 18337, 20000,
      30656, 30657, 36000, 50000, 60000, 65535)
CUS = (256, 304)
HINTS = ((-1, 0), (100, 300), (700, 255), (700, 256), (2000, 1000), (5000, 256))   # (ntg_hint, group_hint)
OVERRIDES = ("-", "np=1", "np=2", "half=0", "half=1", "hyb=0", "tgmax=-1", "tgmax=0", "tgmax=64", "tgmax=1000", "tgmax=4094",
             "list=0", "list=64", "solo=0", "split=1", "split=2", "split=4", "waves=4", "waves=12", "wpb=1", "wpb=8")
FIELDS = ("np", "wpb", "lds_bytes", "perpair_bytes", "opts", "half_items", "stride", "split")
LDS_CAP = 160 * 1024
CNT_BYTES = 2             # ICIKT_CNT_BYTES
TL_BYTES = 2112           # K1_TL_BYTES


def n_pairs_axis(n_cu):
    """Each border of the plan in the pair count, and the value one past it: 1 | 2 pairs; tasks = (n_pairs + 1) / 2 <=
    n_cu; 2 * tasks <= 5 * n_cu; n_pairs <= 4 * n_cu; 256 and 1 024 columns."""
    return (1, 2, 2 * n_cu, 2 * n_cu + 1, 5 * n_cu, 5 * n_cu + 1, 4 * n_cu, 4 * n_cu + 1, 32640, 32641, 523776, 523777)


def plan_cases(n_cu):
    return [(n, p, tied, ntg, grp) for n in NS for p in n_pairs_axis(n_cu) for tied in (0, 1) for ntg, grp in HINTS]


def plan_lines(ov, n_cu):
    return [f"plan {n} {p} {n_cu} {tied} {ntg} {grp} {ov}" for n, p, tied, ntg, grp in plan_cases(n_cu)]


PLAN_GROUPS = [(ov, n_cu) for ov in OVERRIDES for n_cu in CUS]

# ---- the tie verdict ----
N_SHORT, N_LONG = 20000, 40000     # 11 words per lane of a half's prefix rebuild; too long for the half-wave kernels


def stats(sizes=(), fill=0, ngroups=1000, nna=0):
    """The six fields tie_verdict reads of a column whose values other than the fill hold tie groups of `sizes` rows
    and whose fill group has `fill` rows: (ntg, tfill, e0, e1, ngroups, nna)."""
    allg = list(sizes) + ([fill] if fill >= 2 else [])
    e0 = sum(t * (t - 1) for t in allg)
    e1 = sum(t * (t - 1) * (t - 2) for t in allg)
    return (len(allg), fill, e0, e1, ngroups, nna)


# (columns, verdict for short columns, verdict for long columns); a verdict: (tied_state, ntg_hint, group_hint), None
# where only the fixture says.  rows = sum(n - nna), all_groups = sum(max(ngroups, 1)), groups = sum(ntg), m = columns.
TIED_CASES = [
    # groups == 8 m: not tied; one more group: tied (short: the half-wave kernels; long with ~1 000 values per column:
    # 40 rows per group, two pairs per wave stay)
    ([stats([3] * 8), stats([3] * 8)], (0, 8, 3), (0, 8, 3)),
    ([stats([3] * 9), stats([3] * 8)], (1, 9, 3), (0, 9, 3)),
    ([stats([3] * 7), stats([3] * 8)], (0, 8, 3), (0, 8, 3)),
    # the same with a fill group: it is a tie group of the column's list, and no part of a tied pair's group size
    ([stats([3] * 7, fill=50, nna=50)], (0, 8, 3), (0, 8, 3)),
    ([stats([3] * 8, fill=50, nna=50)], (1, 9, 3), (0, 9, 3)),
    ([stats([3] * 8, fill=50, nna=50), stats([3] * 8)], (1, 9, 3), (0, 9, 3)),      # 17 > 16
    ([stats([3] * 8, fill=50, nna=50), stats([3] * 7)], (0, 9, 3), (0, 9, 3)),      # 16 == 16
    # rows == 32 all_groups (long columns, tied): 2 x 40 000 rows over 2 500 | 2 501 | 2 499 values
    ([stats([16] * 20, ngroups=1250), stats([16] * 20, ngroups=1250)], (1, 20, 16), (0, 20, 16)),
    ([stats([16] * 20, ngroups=1250), stats([16] * 20, ngroups=1251)], (1, 20, 16), (1, 20, 16)),
    ([stats([16] * 20, ngroups=1249), stats([16] * 20, ngroups=1250)], (1, 20, 16), (0, 20, 16)),
    # ... with missing rows: 79 968 rows over 2 499 values (equal), over 2 500 (below)
    ([stats([16] * 20, fill=32, ngroups=1249, nna=32), stats([16] * 20, ngroups=1250)], (1, 21, 16), (0, 21, 16)),
    ([stats([16] * 20, fill=32, ngroups=1250, nna=32), stats([16] * 20, ngroups=1250)], (1, 21, 16), (1, 21, 16)),
    # g0 == 0: nothing tied but the fill group -> no group size; one tied pair beside it -> 2
    ([stats([], fill=100, nna=100)], (0, 1, 0), (0, 1, 0)),
    ([stats([2], fill=100, nna=100)], (0, 2, 2), (0, 2, 2)),
    ([stats([])], (0, 0, 0), (0, 0, 0)),
    ([stats([2])], (0, 1, 2), (0, 1, 2)),
    # the group size plan_k1 compares with 256, fill group apart
    ([stats([255] * 40, ngroups=60)], (1, 40, 255), (0, 40, 255)),
    ([stats([256] * 40, ngroups=60)], (1, 40, 256), (0, 40, 256)),
    ([stats([256] * 40, fill=5000, ngroups=60, nna=5000)], (1, 41, 256), (0, 41, 256)),
    ([stats([256] * 40, fill=5000, ngroups=60, nna=5000), stats([3] * 2000, ngroups=9000)], (1, 2000, None), None),
    # the clamps: 2^20 tie groups, a group of 10^6 rows; a column without a value; more missing rows than rows
    ([(1 << 21, 0, 1 << 22, 0, 1 << 21, 0)], (1, 1 << 20, 2), (1, 1 << 20, 2)),
    ([stats([1500000] + [3] * 8, ngroups=9)], (1, 9, 1000000), (0, 9, 1000000)),
    ([stats([3] * 9, ngroups=0)], (1, 9, 3), (0, 9, 3)),
    ([stats([3] * 9, ngroups=2000, nna=50000)], (1, 9, 3), (1, 9, 3)),                # no rows: 0 < 32 x 2 000
    # 64 columns, one group past 8 per column on average
    ([stats([4] * 8, ngroups=5000)] * 63 + [stats([4] * 9, ngroups=5000)], (1, 9, 4), (1, 9, 4)),
    ([stats([4] * 8, ngroups=5000)] * 64, (0, 8, 4), (0, 8, 4)),
]


def tied_lines():
    out = []
    for cols, _, _ in TIED_CASES:
        flat = " ".join(str(v) for c in cols for v in c)
        for long_cols, n in ((0, N_SHORT), (1, N_LONG)):
            out.append(f"tied {long_cols} {n} {len(cols)} {flat}")
    return out


# ---- the task lists ----
COMBN_RANGES = [(5, 0, 10), (7, 3, 17), (7, 7, 20), (7, 6, 11), (7, 20, 21), (7, 0, 21), (7, 5, 5), (2, 0, 1)]


def combn_ref(S, begin, end):
    iu, ju = np.triu_indices(S, k=1)
    return [int(v) for v in iu[begin:end]], [int(v) for v in ju[begin:end]]


def shuffled(pi, pj, seed):
    """A fixed permutation of a list (Fisher-Yates over a 31-bit linear congruential sequence)."""
    idx, x = list(range(len(pi))), seed
    for k in range(len(idx) - 1, 0, -1):
        x = (1103515245 * x + 12345) % (1 << 31)
        r = x % (k + 1)
        idx[k], idx[r] = idx[r], idx[k]
    return [pi[k] for k in idx], [pj[k] for k in idx]


def pair_lists():
    """name -> (pi, pj)"""
    L = {}
    L["combn5"] = combn_ref(5, 0, 10)
    L["combn7_mid_a"] = combn_ref(7, 3, 17)
    L["combn7_mid_b"] = combn_ref(7, 7, 20)
    # diag_good = FALSE: every sample with itself, appended behind all pairs
    pi, pj = combn_ref(5, 0, 10)
    L["diag5"] = (pi + list(range(5)), pj + list(range(5)))
    # an include_only subset of combn(8, 2): row 0 without its partner row 1, rows 2 and 3 with streamed columns the
    # other lacks, row 5 without row 4, rows 6 and 7 (the last, a single pair beside no partner)
    pi, pj = combn_ref(8, 0, 28)
    keep = [(i, j) for i, j in zip(pi, pj) if i in (0, 2, 3, 5, 6) and (i, j) not in ((3, 6), (2, 5), (2, 3))]
    L["include8"] = ([i for i, _ in keep], [j for _, j in keep])
    for name in ("combn5", "combn7_mid_a", "diag5", "include8"):
        L[name + "_shuffled"] = shuffled(*L[name], seed=len(L))
    L["one"] = ([0], [1])
    L["none"] = ([], [])
    return L


def units_lines():
    """[(name, np, line)]"""
    out = []
    for name, (pi, pj) in pair_lists().items():
        for np_ in (1, 2):
            out.append((name, np_, " ".join(str(v) for v in ["units", np_, len(pi), *pi, *pj])))
    return out


# ---- the grid of a launch ----
# (np, half_items, wpb, split, opts), count, per_cu, n_cu, gridmult, gridcap -> [split, opts, blocks, persistent]
WHOLE = (2, 0, 4, 0, 4)       # two long-column pairs per wave, four waves per workgroup: K1_OPT_HALF_LAYOUT
SINGLE = (1, 0, 1, 0, 0)      # one pair per wave, single-wave workgroups
HALF = lambda split: (2, 5, 4, split, 1)   # a half-wave plan (K1_OPT_HALF), tasks cut in `split` segments
GRID_CASES = [
    # want = ceil(count / wpb) below, at and above cap = per_cu x CUs = 512
    ((WHOLE, 4, 2, 256, -1, -1), [1, 4, 1, 0]),
    ((WHOLE, 2044, 2, 256, -1, -1), [1, 4, 511, 0]),
    ((WHOLE, 2048, 2, 256, -1, -1), [1, 4, 512, 0]),
    ((WHOLE, 2049, 2, 256, -1, -1), [1, 4, 512, 1]),
    ((WHOLE, 1000000, 2, 256, -1, -1), [1, 4, 512, 1]),
    ((WHOLE, 1000000, 3, 304, -1, -1), [1, 4, 912, 1]),
    ((SINGLE, 6144, 24, 256, -1, -1), [1, 0, 6144, 0]),
    ((SINGLE, 6145, 24, 256, -1, -1), [1, 0, 6144, 1]),
    # gridcap = 1: one workgroup runs every task; a launch of one workgroup is not persistent
    ((WHOLE, 4, 2, 256, -1, 1), [1, 4, 1, 0]),
    ((WHOLE, 5, 2, 256, -1, 1), [1, 4, 1, 1]),
    ((SINGLE, 100, 24, 256, -1, 1), [1, 0, 1, 1]),
    # gridmult = 2: twice what the chip holds; gridcap caps the product
    ((WHOLE, 4096, 2, 256, 2, -1), [1, 4, 1024, 0]),
    ((WHOLE, 4097, 2, 256, 2, -1), [1, 4, 1024, 1]),
    ((WHOLE, 4097, 2, 256, 2, 100), [1, 4, 100, 1]),
    ((WHOLE, 4097, 2, 256, 0, 0), [1, 4, 512, 1]),                # 0: the library's choice, like -1
    # half-wave plans: one wave per segment, never persistent -- whatever the caps say
    ((HALF(1), 1000, 0, 256, -1, -1), [1, 1, 250, 0]),
    ((HALF(2), 1000, 0, 256, -1, -1), [2, 1 | 1 << 4, 500, 0]),
    ((HALF(4), 1000, 0, 256, -1, -1), [4, 1 | 2 << 4, 1000, 0]),
    ((HALF(4), 1001, 0, 256, -1, -1), [4, 1 | 2 << 4, 1001, 0]),
    ((HALF(2), 1001, 0, 256, -1, -1), [2, 1 | 1 << 4, 501, 0]),
    ((HALF(1), 10000000, 0, 256, -1, 1), [1, 1, 2500000, 0]),
    ((HALF(4), 10000000, 0, 256, 2, 1), [4, 1 | 2 << 4, 10000000, 0]),
    ((HALF(1), 1, 0, 256, -1, -1), [1, 1, 1, 0]),
    # segments are the half-wave kernels': a whole-wave plan ignores the field
    (((2, 0, 4, 4, 4), 2049, 2, 256, -1, -1), [1, 4, 512, 1]),
    (((1, 0, 4, 2, 0), 2048, 2, 256, -1, -1), [1, 0, 512, 0]),
]


def grid_lines():
    return ["grid " + " ".join(str(v) for v in [*pl, *rest]) for (pl, *rest), _ in GRID_CASES]


def all_lines():
    """Every case, in the order of the program's output: {section: lines}."""
    return {"plan": [l for g in PLAN_GROUPS for l in plan_lines(*g)], "tied": tied_lines(),
            "combn": [f"combn {S} {b} {e}" for S, b, e in COMBN_RANGES], "units": [l for _, _, l in units_lines()],
            "grid": grid_lines()}


def digest(rows):
    return hashlib.sha256(("\n".join(rows) + "\n").encode()).hexdigest()


def compile_printer(src, out, extra=()):
    """Build the program, with the sanitizers where they link."""
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, *extra, src, "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:   # (no sanitizer runtime here)
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def run_sections(prog):
    """{section: the printed lines} of every case, from one run of the program."""
    sections = all_lines()
    r = subprocess.run([prog], input="\n".join(l for ls in sections.values() for l in ls) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) - 1 == sum(len(ls) for ls in sections.values())
    got, at = {}, 0
    for name, ls in sections.items():
        got[name] = out[at:at + len(ls)]
        at += len(ls)
    return got


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("k1plan") / "k1plan_print")
    compile_printer(SRC, out)
    return out


@pytest.fixture(scope="module")
def got(prog):
    return run_sections(prog)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def plan_group(got, ov, n_cu):
    k = PLAN_GROUPS.index((ov, n_cu))
    per = len(plan_cases(n_cu))
    return got["plan"][k * per:(k + 1) * per]


def test_header_compiles_alone(tmp_path):
    """icikt_k1plan.h is host arithmetic: the host compiler takes it by itself, warnings as errors."""
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "icikt_k1plan.h"\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-fsyntax-only", str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_plan_rows_of_the_library_s_choice(got, golden):
    """Every field of every plan the library chooses on 256 CUs."""
    rows = [json.loads(l) for l in plan_group(got, "-", 256)]
    assert len(rows) == len(golden["plan_rows"]) == len(plan_cases(256))
    for case, g, w in zip(plan_cases(256), rows, golden["plan_rows"]):
        assert g == w, (case, dict(zip(FIELDS, g)), dict(zip(FIELDS, w)))


@pytest.mark.parametrize("ov,n_cu", PLAN_GROUPS, ids=[f"{ov}@{n_cu}" for ov, n_cu in PLAN_GROUPS])
def test_plan_grid(got, golden, ov, n_cu):
    rows = plan_group(got, ov, n_cu)
    assert digest(rows) == golden["plan_sha256"][f"{ov}@{n_cu}"]
    # whatever the plan decides, the launch must fit a CU and the kernel's layout must fit the bytes of a pair
    for case, row in zip(plan_cases(n_cu), rows):
        p = dict(zip(FIELDS, json.loads(row)))
        n = case[0]
        Wp = (n + 63) // 64 + 1
        assert p["np"] in (1, 2) and 1 <= p["wpb"] <= 8, (case, p)
        assert p["lds_bytes"] == p["wpb"] * p["np"] * p["perpair_bytes"] <= LDS_CAP, (case, p)
        cap, tg_list = p["opts"] >> 18, (p["opts"] >> 8) & 0x3FF
        assert 0 <= cap <= 4094 and 0 <= tg_list <= 256, (case, p)
        if p["half_items"] > 0:
            hi = (Wp + 31) >> 5
            hi = hi + 1 if hi >= 8 and hi % 2 == 0 else hi
            assert p["np"] == 2 and p["opts"] & 1 and p["half_items"] == hi <= 15 and p["stride"] == 32 * hi, (case, p)
            assert p["split"] in (1, 2, 4), (case, p)
            pre = 32 * (16 if hi > 8 else 8) * 2
            assert p["perpair_bytes"] % 16 == 0 and p["perpair_bytes"] >= p["stride"] * 8 + pre + CNT_BYTES * (cap + 2), (case, p)
        else:
            assert not p["opts"] & 1 and p["stride"] == (Wp + 7) // 8 * 8, (case, p)
            table = CNT_BYTES * (cap + 2) if cap > 0 else 0
            assert p["perpair_bytes"] >= p["stride"] * 8 + TL_BYTES + table, (case, p)
        if ov.startswith("np="):
            assert p["np"] == int(ov[3:]), (case, p)
        if ov.startswith("wpb="):
            assert p["wpb"] <= int(ov[4:]), (case, p)
        if ov == "tgmax=-1":
            assert p["opts"] & 2 and cap == 0 and tg_list == 0, (case, p)
        if ov.startswith("list="):
            assert tg_list <= int(ov[5:]), (case, p)
        if ov == "solo=0":
            assert p["opts"] & 8, (case, p)
        if ov.startswith("split=") and p["half_items"] > 0:
            assert p["split"] == int(ov[6:]), (case, p)


def test_tie_verdict(got, golden):
    assert [json.loads(l) for l in got["tied"]] == golden["tied"]
    rows = iter(json.loads(l) for l in got["tied"])
    for k, (cols, short, long_) in enumerate(TIED_CASES):
        for want in (short, long_):
            g = next(rows)
            for a, b in zip(g, want or ()):
                assert b is None or a == b, (k, g, want)


def test_combn_ranges(got, golden):
    assert [json.loads(l) for l in got["combn"]] == golden["combn"]
    for (S, b, e), l in zip(COMBN_RANGES, got["combn"]):
        assert json.loads(l) == list(combn_ref(S, b, e)), (S, b, e)


def test_task_lists(got, golden):
    lists = pair_lists()
    for (name, np_, _), l in zip(units_lines(), got["units"]):
        u = json.loads(l)
        assert u == golden["units"][f"{name}@np{np_}"], (name, np_)
        pi, pj = lists[name]
        tasks = list(zip(u[0::2], u[1::2]))
        # every pair index in exactly one task
        assert sorted(p for t in tasks for p in t if p >= 0) == list(range(len(pi))), (name, np_)
        assert all(a >= 0 for a, _ in tasks), (name, np_)
        if np_ == 1:
            assert tasks == [(p, -1) for p in range(len(pi))], name
        for a, b in tasks:
            if b >= 0:   # the two gathered columns of one block of the rec table, one streamed column
                assert pi[a] % 2 == 0 and pi[b] == pi[a] + 1 and pj[a] == pj[b], (name, a, b)
    # the lists are what they are meant to be: both paths of build_units, pairs with and without a partner
    by = {(name, np_): json.loads(l) for (name, np_, _), l in zip(units_lines(), got["units"])}
    assert len(by[("combn5", 2)]) // 2 == 6 and len(by[("include8", 2)]) // 2 < len(lists["include8"][0])
    for name in ("combn5", "combn7_mid_a", "include8"):   # a shuffled list pairs up as many as the sorted one
        assert len(by[(name, 2)]) == len(by[(name + "_shuffled", 2)]), name


def test_grid(got, golden):
    assert [json.loads(l) for l in got["grid"]] == golden["grid"]
    for (case, want), l in zip(GRID_CASES, got["grid"]):
        assert json.loads(l) == want, case


# ---- the pipelined host entries' task slices: tasks by the chunk in which their last column arrives ----
# tests/golden/pipeline_parent.json holds what the code printed while it stood inline in upload_prepare_pairs
# (icikt_capi.cpp): that function's chunk callback for the full triangle and its counting sort over build_units' list were
# compiled as they were into a stand-alone program beside the parent's icikt_k1plan.h, and run once on the cases below.
#   triangle_sha256   {"chunkunits" | "chunkorder": SHA-256 of the rows of every triangle case, in triangle_cases() order}
#   chunkorder        {"<list>@np<np>@<ends>": [first, units]} of the explicit lists
PIPE_GOLDEN = os.path.join(ROOT, "tests", "golden", "pipeline_parent.json")
TRIANGLE_S = range(2, 42)


def chunk_ends(S):
    """Ways to cut S columns into chunks, as the chunks' ends (the last one is S): a single chunk, one-column chunks,
    even and odd widths, an odd first chunk ahead of even ones, uneven thirds."""
    pats = [[S], list(range(1, S + 1))]
    pats += [list(range(w, S, w)) + [S] for w in (2, 4, 6, 16, 3, 5, 7, 15)]
    pats += [list(range(1, S, 2)) + [S], list(range(3, S, 4)) + [S], sorted({max(1, S // 3), max(1, S // 2), S})]
    out = []
    for p in pats:
        if p not in out:
            out.append(p)
    return out


def triangle_cases():
    return [(S, np_, ends) for S in TRIANGLE_S for np_ in (1, 2) for ends in chunk_ends(S)]


def explicit_lists():
    """name -> (pi, pj, S): a subset of the pairs i <= j of S columns -- self pairs among them -- each in either
    orientation, shuffled: build_units takes its unsorted branch."""
    L = {}
    for S, per_mille, seed in ((7, 1000, 3), (12, 600, 5), (20, 500, 7), (33, 350, 11)):
        iu, ju = np.triu_indices(S, k=0)
        pi, pj, x = [], [], seed
        for i, j in zip(iu, ju):
            x = (1103515245 * x + 12345) % (1 << 31)
            if (x >> 8) % 1000 >= per_mille:
                continue
            x = (1103515245 * x + 12345) % (1 << 31)
            i, j = (int(j), int(i)) if (x >> 8) & 1 else (int(i), int(j))
            pi.append(i)
            pj.append(j)
        L[f"list{S}"] = (*shuffled(pi, pj, seed), S)
    return L


def explicit_ends(S):
    return [[S], list(range(1, S + 1)), list(range(2, S, 2)) + [S], list(range(5, S, 5)) + [S], list(range(1, S, 2)) + [S]]


def explicit_cases():
    return [(name, np_, ends) for name, (_, _, S) in explicit_lists().items() for np_ in (1, 2) for ends in explicit_ends(S)]


def chunkorder_line(np_, pi, pj, ends):
    return " ".join(str(v) for v in ["chunkorder", np_, len(pi), *pi, *pj, len(ends), *ends])


def chunk_lines():
    """{section: lines}, in the order of the program's output."""
    lists = explicit_lists()
    tri = {S: combn_ref(S, 0, S * (S - 1) // 2) for S in TRIANGLE_S}
    return {
        "tri_units": [" ".join(str(v) for v in ["chunkunits", S, np_, len(ends), *ends]) for S, np_, ends in triangle_cases()],
        "tri_order": [chunkorder_line(np_, *tri[S], ends) for S, np_, ends in triangle_cases()],
        "tri_build": [" ".join(str(v) for v in ["units", np_, len(tri[S][0]), *tri[S][0], *tri[S][1]])
                      for S in TRIANGLE_S for np_ in (1, 2)],
        "list_order": [chunkorder_line(np_, *lists[name][:2], ends) for name, np_, ends in explicit_cases()],
        "list_build": [" ".join(str(v) for v in ["units", np_, len(lists[name][0]), *lists[name][0], *lists[name][1]])
                       for name in lists for np_ in (1, 2)],
    }


def run_chunk_sections(prog):
    sections = chunk_lines()
    r = subprocess.run([prog], input="\n".join(l for ls in sections.values() for l in ls) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) - 1 == sum(len(ls) for ls in sections.values())
    got, at = {}, 0
    for name, ls in sections.items():
        got[name] = out[at:at + len(ls)]
        at += len(ls)
    return got


@pytest.fixture(scope="module")
def chunks(prog):
    return run_chunk_sections(prog)


@pytest.fixture(scope="module")
def pipe_golden():
    with open(PIPE_GOLDEN) as f:
        return json.load(f)


def by_chunk(units, pi, pj, ends):
    """[first, units] as the rule states it: the tasks of build_units' list whose last column lies in [ends[q-1],
    ends[q]), chunk after chunk, in build_units' order inside a chunk."""
    groups = [[] for _ in ends]
    for t in zip(units[0::2], units[1::2]):
        last = max(max(pi[p], pj[p]) for p in t if p >= 0)
        groups[next(q for q, e in enumerate(ends) if last < e)].append(t)
    first = [0]
    for g in groups:
        first.append(first[-1] + len(g))
    return [first, [p for g in groups for t in g for p in t]]


def test_triangle_slices_one_rule(chunks, pipe_golden):
    """For the full triangle the arithmetic producer (combn_chunk_units, chunk after chunk) and the sorting one
    (build_units + order_units_by_chunk) print the same values, the parent's; and those are the rule's: a permutation
    of build_units' list, every task in the chunk of its last column, build_units' order inside a chunk."""
    cases = triangle_cases()
    assert len(cases) >= 800
    assert chunks["tri_units"] == chunks["tri_order"]
    assert digest(chunks["tri_units"]) == pipe_golden["triangle_sha256"]["chunkunits"]
    assert digest(chunks["tri_order"]) == pipe_golden["triangle_sha256"]["chunkorder"]
    built = {(S, np_): json.loads(l) for (S, np_), l in zip(((S, np_) for S in TRIANGLE_S for np_ in (1, 2)), chunks["tri_build"])}
    shapes = set()
    for (S, np_, ends), row in zip(cases, chunks["tri_units"]):
        pi, pj = combn_ref(S, 0, S * (S - 1) // 2)
        assert json.loads(row) == by_chunk(built[(S, np_)], pi, pj, ends), (S, np_, ends)
        shapes |= {"single"} if len(ends) == 1 else set()
        shapes |= {"columns"} if len(ends) == S and S > 1 else set()
        shapes |= {"odd"} if any(e % 2 for e in ends[:-1]) else set()
        shapes |= {"even"} if len(ends) > 1 and not any(e % 2 for e in ends[:-1]) else set()
    assert shapes == {"single", "columns", "odd", "even"}


def test_explicit_list_slices(chunks, pipe_golden):
    lists = explicit_lists()
    for name, (pi, pj, S) in lists.items():
        assert any(i > j for i, j in zip(pi, pj)) and any(i < j for i, j in zip(pi, pj)) and any(i == j for i, j in zip(pi, pj))
        assert list(zip(pi, pj)) != sorted(zip(pi, pj)), name          # the unsorted branch of build_units
    built = {(name, np_): json.loads(l) for (name, np_), l in zip(((n_, p_) for n_ in lists for p_ in (1, 2)), chunks["list_build"])}
    assert len(pipe_golden["chunkorder"]) == len(explicit_cases())
    for (name, np_, ends), row in zip(explicit_cases(), chunks["list_order"]):
        pi, pj, _ = lists[name]
        got = json.loads(row)
        assert got == pipe_golden["chunkorder"][f"{name}@np{np_}@{'-'.join(str(e) for e in ends)}"], (name, np_, ends)
        assert got == by_chunk(built[(name, np_)], pi, pj, ends), (name, np_, ends)
        assert len(got[0]) == len(ends) + 1 and got[0][-1] * 2 == len(got[1])
    for name in lists:   # two pairs per wave do pair up some of a shuffled list
        assert len(built[(name, 2)]) < len(built[(name, 1)]), name
