"""The device-free block arithmetic of the selection entries (csrc/icikt_blocks.h: cut_rows, row_offset, class_index,
the class cursor and the PairBlocks a call walks) against a numpy brute force, without a GPU and without the library:
tests/blocks_print.cpp is compiled with the host compiler (with the address and undefined-behaviour sanitizers where
they link) and prints what the header makes of the cases on its command line."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.medians_checker import class_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "blocks_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")

ROW_SAMPLES = (1, 2, 3, 4, 5, 64, 65, 130)
ROW_BUDGETS = (1, 2, 3, 7, 1000, 2 ** 24)
CLASS_BUDGETS = (1, 2, 5, 10 ** 6)
CLASS_VECTORS = {
    "one class": [0] * 9,
    "three interleaved": [s % 3 for s in range(13)],
    "a singleton in the middle": [0, 0, 1, 0, 2, 1, 1, 0],
    "all singletons": list(range(6)),
    "sizes 2 and 11": [1, 0, 1] + [1] * 8 + [0] + [1],
}


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("blocks") / "blocks_print")
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


@pytest.mark.parametrize("S", ROW_SAMPLES)
def test_cut_rows(prog, S):
    got = prog("rows", S, *ROW_BUDGETS)
    iu, ju = np.triu_indices(S, k=1)
    total = len(iu)
    # row_offset: the first pair of row i in combn order (the last row has none: the end of the triangle)
    assert got["row_offset"] == [int(np.searchsorted(iu, i)) for i in range(S)]
    assert [c["budget"] for c in got["cuts"]] == list(ROW_BUDGETS)
    for cut in got["cuts"]:
        budget, blocks = cut["budget"], cut["blocks"]
        assert cut["total"] == total and cut["n_blocks"] == len(blocks)
        assert cut["block_max"] == max([b[1] for b in blocks] + [1])
        row = 0
        for q, (begin, count, first, last, pi, pj) in enumerate(blocks):
            assert first == row and last > first, (S, budget, blocks)      # the rows [0, S - 1) in order, none empty
            assert pi == [] and pj == []
            inside = (iu >= first) & (iu < last)
            assert count == int(inside.sum()) and begin == int(np.argmax(inside))
            if last - first > 1:
                assert count <= budget
                if q < len(blocks) - 1:
                    assert last % 2 == 0, (S, budget, blocks)
            else:   # a single row may exceed the budget
                assert count == S - 1 - first
            row = last
        assert row == max(S - 1, 0)
        assert sum(b[1] for b in blocks) == total
    # the whole triangle is one block under the library's own budget, and a row per block under budget 1
    assert len(got["cuts"][-1]["blocks"]) == (1 if S > 1 else 0)
    assert len(got["cuts"][0]["blocks"]) == max(S - 1, 0)


def _brute_classes(cls):
    cls = np.asarray(cls)
    S = len(cls)
    pos, size, base = np.zeros(S, int), np.zeros(S, int), np.zeros(S, int)
    total = 0
    for k in sorted(set(cls.tolist())):
        members = np.nonzero(cls == k)[0]
        pos[members] = np.arange(len(members))
        size[members] = len(members)
        base[members] = total
        total += len(members) * (len(members) - 1) // 2
    return pos.tolist(), size.tolist(), base.tolist(), total


@pytest.mark.parametrize("name", sorted(CLASS_VECTORS))
def test_class_cursor(prog, name):
    cls = CLASS_VECTORS[name]
    got = prog("classes", len(CLASS_BUDGETS), *CLASS_BUDGETS, *cls)
    pos, size, base, total = _brute_classes(cls)
    assert (got["pos"], got["size"], got["base"], got["total"]) == (pos, size, base, total)
    assert got["member"] == sorted(range(len(cls)), key=lambda s: (cls[s], s))
    want_pi, want_pj = (a.tolist() for a in class_pairs(cls))     # class by class, combn order inside a class
    assert len(want_pi) == total
    for cut in got["cuts"]:
        budget, blocks = cut["budget"], cut["blocks"]
        assert cut["total"] == total and cut["n_blocks"] == len(blocks) == -(-total // budget)
        assert cut["block_max"] == max(1, min(total, budget))
        assert [b[1] for b in blocks[:-1]] == [budget] * (len(blocks) - 1)      # every slice but the last is full
        assert all(0 < b[1] <= budget and len(b[4]) == len(b[5]) == b[1] for b in blocks)
        assert [b[0] for b in blocks] == np.cumsum([0] + [b[1] for b in blocks[:-1]]).tolist()[:len(blocks)]
        assert sum((b[4] for b in blocks), []) == want_pi and sum((b[5] for b in blocks), []) == want_pj


def test_no_class_vector_is_one_class(prog):
    got = prog("classes", 1, 4, "@7")
    assert got["runs"] == [0, 7] and got["member"] == list(range(7)) and got["total"] == 21
    assert got["pos"] == list(range(7)) and got["size"] == [7] * 7 and got["base"] == [0] * 7
    iu, ju = np.triu_indices(7, k=1)
    blocks = got["cuts"][0]["blocks"]
    assert [b[1] for b in blocks] == [4, 4, 4, 4, 4, 1]
    assert sum((b[4] for b in blocks), []) == iu.tolist() and sum((b[5] for b in blocks), []) == ju.tolist()
