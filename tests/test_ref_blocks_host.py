"""The device-free block arithmetic of icikt_ref_cross_* (csrc/icikt_blocks.h: PairBlocks::rect_ref_first,
ref_query_col) and the task list the pair engine builds of such a block (csrc/icikt_k1plan.h: build_units) against a
numpy enumeration, without a GPU and without the library: tests/ref_blocks_print.cpp is compiled with the host compiler
(with the address and undefined-behaviour sanitizers where they link) and prints what the headers make of the cases on
its command line.  The layout is the mirror of icikt_cross_*'s: the reference in device columns 0 .. Sr - 1, the batch
from the next even column on, so a pair is (Sr_even + q, r) with pi > pj."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ref_blocks_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")

QUERIES = (1, 2, 3, 4, 5, 64, 65)
REFERENCES = (1, 2, 7, 130)


def budgets(Sr):
    return (1, 2, Sr, 2 * Sr, 3 * Sr + 1, 2 ** 24)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ref_blocks") / "ref_blocks_print")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:   # (no sanitizer runtime here)
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr

    def run(*args):
        r = subprocess.run([out, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    return run


def expected_tasks(first, last, Sr):
    """build_units(np = 2) of query rows [first, last), block-relative pair indices: the rows 2a and 2a + 1, both
    inside, share every reference column (Sr tasks of two pairs); any other row runs alone (Sr tasks of one pair)."""
    tasks, q = [], first
    while q < last:
        at = (q - first) * Sr
        if q % 2 == 0 and q + 1 < last:
            tasks += [w for r in range(Sr) for w in (at + r, at + Sr + r)]
            q += 2
        else:
            tasks += [w for r in range(Sr) for w in (at + r, -1)]
            q += 1
    return tasks


@pytest.mark.parametrize("Sr", REFERENCES)
@pytest.mark.parametrize("Sq", QUERIES)
def test_ref_first_blocks(prog, Sq, Sr):
    got = prog(Sq, Sr, *budgets(Sr))
    q0 = Sr + (Sr & 1)
    assert got["query_col"] == q0 and q0 % 2 == 0
    # the call's pair order: query-major, p = q * Sr + r, as device columns (q0 + q, r)
    want_pi = q0 + np.repeat(np.arange(Sq), Sr)
    want_pj = np.tile(np.arange(Sr), Sq)
    assert [c["budget"] for c in got["cuts"]] == list(budgets(Sr))
    for cut in got["cuts"]:
        budget, blocks = cut["budget"], cut["blocks"]
        assert cut["total"] == Sq * Sr and cut["n_blocks"] == len(blocks)
        assert cut["block_max"] == max([b[1] for b in blocks] + [1])
        # the cut is cut_rect_rows'
        assert [[b[2], b[3]] for b in blocks] == cut["rows"]
        row, seen = 0, []
        for begin, count, first, last, pi, pj, units in blocks:
            assert first == row and last > first, (Sq, Sr, budget)
            assert begin == first * Sr and count == (last - first) * Sr
            if last - first > 1:
                assert count <= budget
                if last < Sq:
                    assert last % 2 == 0, (Sq, Sr, budget, blocks)
            assert pi == want_pi[begin:begin + count].tolist() and pj == want_pj[begin:begin + count].tolist()
            assert all(a > b for a, b in zip(pi, pj))
            keys = list(zip(pi, pj))
            assert keys == sorted(keys)                                   # sorted by (pi, pj)
            seen += keys
            assert units == expected_tasks(first, last, Sr), (Sq, Sr, budget, first, last)
            row = last
        assert row == Sq
        # every pair once, in query-major order
        assert seen == [(q0 + q, r) for q in range(Sq) for r in range(Sr)]
    assert len(got["cuts"][-1]["blocks"]) == 1
    assert len(got["cuts"][0]["blocks"]) == Sq
    assert all(u == -1 for b in got["cuts"][0]["blocks"] for u in b[6][1::2])


def test_row_pairs_share_every_reference_column(prog):
    """Query rows [2a, 2a + 2) give exactly Sr tasks of two pairs over the same reference column; a trailing odd row
    gives Sr single tasks."""
    Sr = 7
    got = prog(5, Sr, 2 * Sr)
    q0 = 8
    blocks = got["cuts"][0]["blocks"]
    assert [(b[2], b[3]) for b in blocks] == [(0, 2), (2, 4), (4, 5)]
    for begin, count, first, last, pi, pj, units in blocks[:2]:
        pairs = list(zip(units[0::2], units[1::2]))
        assert len(pairs) == Sr and all(y == x + Sr for x, y in pairs)
        assert all(pi[x] == q0 + first and pi[y] == q0 + first + 1 and pj[x] == pj[y] for x, y in pairs)
    tail = blocks[2][6]
    assert tail[0::2] == list(range(Sr)) and tail[1::2] == [-1] * Sr
