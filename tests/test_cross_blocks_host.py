"""The device-free block arithmetic of icikt_cross_* (csrc/icikt_blocks.h: PairBlocks::rect, cut_rect_rows,
rect_ref_col) and the task list the pair engine builds of such a block (csrc/icikt_k1plan.h: build_units) against a
numpy enumeration, without a GPU and without the library: tests/cross_blocks_print.cpp is compiled with the host
compiler (with the address and undefined-behaviour sanitizers where they link) and prints what the headers make of the
cases on its command line."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cross_blocks_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")

QUERIES = (1, 2, 3, 4, 5, 64, 65)
REFERENCES = (1, 2, 7, 130)


def budgets(Sr):
    return (1, 2, Sr, 2 * Sr, 3 * Sr + 1, 2 ** 24)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cross_blocks") / "cross_blocks_print")
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
    """build_units(np = 2) of rows [first, last), block-relative pair indices: the rows 2a and 2a + 1, both inside, share
    every reference column (Sr tasks of two pairs); any other row runs alone (Sr tasks of one pair)."""
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
def test_rect_blocks(prog, Sq, Sr):
    got = prog(Sq, Sr, *budgets(Sr))
    ref_col = Sq + (Sq & 1)
    assert got["ref_col"] == ref_col and ref_col % 2 == 0
    # the call's pair order: query-major, p = q * Sr + r, as device columns (q, ref_col + r)
    want_pi = np.repeat(np.arange(Sq), Sr)
    want_pj = ref_col + np.tile(np.arange(Sr), Sq)
    assert [c["budget"] for c in got["cuts"]] == list(budgets(Sr))
    for cut in got["cuts"]:
        budget, blocks = cut["budget"], cut["blocks"]
        assert cut["total"] == Sq * Sr and cut["n_blocks"] == len(blocks)
        assert cut["block_max"] == max([b[1] for b in blocks] + [1])
        row = 0
        for n, (begin, count, first, last, pi, pj, units) in enumerate(blocks):
            assert first == row and last > first, (Sq, Sr, budget)        # the rows [0, Sq) in order, none empty
            assert begin == first * Sr and count == (last - first) * Sr    # whole rows, at their place
            if last - first > 1:
                assert count <= budget
                if last < Sq:
                    assert last % 2 == 0, (Sq, Sr, budget, blocks)
            assert pi == want_pi[begin:begin + count].tolist() and pj == want_pj[begin:begin + count].tolist()
            assert units == expected_tasks(first, last, Sr), (Sq, Sr, budget, first, last)
            row = last
        assert row == Sq
        assert sum(b[1] for b in blocks) == Sq * Sr
        # a block holds as many rows as the budget lets it (one less where it must end on an even row)
        fit = max(1, budget // Sr)
        for (_b, _c, first, last, *_rest) in blocks:
            assert last - first in (min(fit, Sq - first), min(fit, Sq - first) - 1)
    # one block under the library's own budget, a row per block under budget 1 (no row is paired then)
    assert len(got["cuts"][-1]["blocks"]) == 1
    assert len(got["cuts"][0]["blocks"]) == Sq
    assert all(u == -1 for b in got["cuts"][0]["blocks"] for u in b[6][1::2])


def test_row_pairs_share_every_reference_column(prog):
    """Rows [2a, 2a + 2) give exactly Sr tasks of two pairs; a trailing odd row gives Sr single tasks."""
    Sr = 7
    got = prog(5, Sr, 2 * Sr)
    blocks = got["cuts"][0]["blocks"]
    assert [(b[2], b[3]) for b in blocks] == [(0, 2), (2, 4), (4, 5)]
    for begin, count, first, last, pi, pj, units in blocks[:2]:
        pairs = list(zip(units[0::2], units[1::2]))
        assert len(pairs) == Sr and all(y == x + Sr for x, y in pairs)
        assert all(pi[x] == first and pi[y] == first + 1 and pj[x] == pj[y] for x, y in pairs)
    tail = blocks[2][6]
    assert tail[0::2] == list(range(Sr)) and tail[1::2] == [-1] * Sr
