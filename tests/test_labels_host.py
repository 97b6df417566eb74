"""The device-free half of the permutation-test entries' labellings (csrc/icikt_labels.h: label_batches,
stage_labellings, first_bad_label) against numpy, without a GPU and without the library: tests/labels_print.cpp is
compiled with the host compiler (with the address and undefined-behaviour sanitizers where they link) and prints what
the header makes of the cases on its command line."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "labels_print.cpp")
CSRC = os.path.join(ROOT, "icikendalltau_amd", "csrc")

PB = 16                    # ANO_PB
PERMS_MAX = 1 << 20        # ANO_PERMS_MAX
BATCH_BYTES = 64 << 20     # ANO_BATCH_BYTES
FILL = 0xFFFF              # what labels_print fills the stage with before every batch

SAMPLES = (1, 2, 3, 17)
CLASSES = (1, 3)
LABELLINGS = (1, 15, 16, 17, 33)
OVERRIDES = (0, 1, 3, 16, 17)   # 0: no anoperms key


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("labels") / "labels_print")
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


def labellings(S, C, n_lab, seed=0):
    """[n_lab, S] labels in 0 .. C - 1; some classes stay empty in some labellings."""
    rng = np.random.default_rng([S, C, n_lab, seed])
    return rng.integers(0, C, size=(n_lab, S)).astype(np.int64)


def stage(prog, labs, C, override, within):
    n_lab, S = labs.shape
    return prog("stage", S, C, n_lab, override, int(within), *labs.ravel().tolist())


def expected_batch(S, n_lab, override):
    """anosim's plan at the sizes of these cases: 64 MB / (2 S) labellings is far past n_lab, so n_lab or the key."""
    return min(override if override > 0 else n_lab, n_lab)


@pytest.mark.parametrize("override", OVERRIDES)
@pytest.mark.parametrize("n_lab", LABELLINGS)
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("S", SAMPLES)
def test_stage_layout_and_within(prog, S, C, n_lab, override):
    """Slot (g, s, p) of a batch's stage is labs[q0 + g 16 + p, s], the unused slots of the last group are 0, nothing
    behind the batch's groups is written, and within is the sum over the classes of C(size, 2), empty classes included."""
    labs = labellings(S, C, n_lab)
    got = stage(prog, labs, C, override, True)
    batch = expected_batch(S, n_lab, override)
    assert got["batch"] == batch
    starts = list(range(0, n_lab, batch))
    assert [b["q0"] for b in got["batches"]] == starts
    for b in got["batches"]:
        q0, nb = b["q0"], b["nb"]
        assert nb == min(batch, n_lab - q0) and b["bad"] is None
        groups = -(-nb // PB)
        want = np.zeros((groups * PB, S), dtype=np.int64)        # labelling-major, padded with labelling 0s
        want[:nb] = labs[q0:q0 + nb]
        want = want.reshape(groups, PB, S).transpose(0, 2, 1)    # [g][s][p]
        assert np.array_equal(np.array(b["stage"], dtype=np.int64).reshape(groups, S, PB), want), (S, C, n_lab, override, q0)
        sizes = np.stack([np.bincount(l, minlength=C) for l in labs[q0:q0 + nb]])
        assert b["within"] == (sizes * (sizes - 1) // 2).sum(axis=1).tolist()
    # without within the stage is the same
    plain = stage(prog, labs, C, override, False)
    assert [b["stage"] for b in plain["batches"]] == [b["stage"] for b in got["batches"]]
    assert all(b["within"] == [] for b in plain["batches"])


def test_within_counts_empty_classes(prog):
    """Five classes of sizes 4, 0, 1, 0, 2: C(4, 2) + C(1, 2) + C(2, 2) = 6 + 0 + 1."""
    labs = np.array([[0, 4, 0, 2, 0, 4, 0]], dtype=np.int64)
    assert stage(prog, labs, 5, 0, True)["batches"][0]["within"] == [7]


BAD_CASES = [          # (q, s) of the bad label in a call of 33 labellings over 17 samples, anoperms = 16
    (0, 0), (0, 16),               # the observed labelling, first and last sample
    (1, 0), (5, 16), (15, 7),      # the first batch
    (16, 0), (16, 16),             # the first labelling of the second batch
    (32, 3),                       # the third batch
]


@pytest.mark.parametrize("value", (-1, 3))
@pytest.mark.parametrize("q,s", BAD_CASES)
def test_bad_label_is_reported_where_it_is(prog, q, s, value):
    S, C, n_lab, batch = 17, 3, 33, 16
    labs = labellings(S, C, n_lab)
    labs[q, s] = value
    got = stage(prog, labs, C, batch, True)
    last = got["batches"][-1]
    assert last["q0"] == q // batch * batch and last["bad"] == [q, s, value]
    assert len(got["batches"]) == q // batch + 1 and all(b["bad"] is None for b in got["batches"][:-1])
    # the labellings of that batch before the bad one are staged, the bad one up to its bad label, nothing behind that
    flat = np.array(last["stage"], dtype=np.int64).reshape(-1, S, PB)
    l_bad = q - last["q0"]
    for l in range(last["nb"]):
        column = flat[l // PB, :, l % PB]
        staged = S if l < l_bad else s if l == l_bad else 0
        assert np.array_equal(column[:staged], labs[last["q0"] + l, :staged]) and np.all(column[staged:] == FILL)


@pytest.mark.parametrize("first,second", [((0, 5), (0, 9)), ((3, 16), (4, 0)), ((15, 2), (16, 1)), ((17, 0), (2, 16))])
def test_the_earlier_of_two_bad_labels_is_reported(prog, first, second):
    """Labelling order, then sample order: the pairs are given in either order of appearance."""
    S, C, n_lab = 17, 3, 33
    labs = labellings(S, C, n_lab, seed=1)
    labs[first] = -1
    labs[second] = C
    q, s = min(first, second)
    assert stage(prog, labs, C, 16, False)["batches"][-1]["bad"] == [q, s, int(labs[q, s])]


PLAN_CASES = [   # (entry, S, C, expected batch before the cut to n_lab)
    ("anosim", 65535, None, 512),
    ("anosim", 100, None, 335536),
    ("anosim", 1, None, 1048576),
    ("permanova", 65535, 2, 64),
    ("permanova", 100, 5, 41936),
    ("permanova", 2, 2500, 1664),
]


@pytest.mark.parametrize("entry,S,C,batch", PLAN_CASES)
def test_batch_plan(prog, entry, S, C, batch):
    """The parent's expressions, by hand.  A labelling costs anosim 2 S bytes and permanova 16 max(S, C); the batch is
    max(16, floor(floor(2^26 / cost) / 16) 16), then at most 2^20 (ANO_PERMS_MAX), then at most n_lab:
      anosim     S = 65 535: 2^26 / 131 070 = 512.003 -> 512, a multiple of 16
                 S = 100:    2^26 / 200 = 335 544.3 -> 335 544 = 20 971 x 16 + 8 -> 335 536
                 S = 1:      2^26 / 2 = 33 554 432 -> the cap 1 048 576
      permanova  S = 65 535, C = 2: 2^26 / 1 048 560 = 64.0003 -> 64
                 S = 100, C = 5:    2^26 / 1 600 = 41 943.04 -> 41 943 = 2 621 x 16 + 7 -> 41 936
                 S = 2, C = 2 500:  2^26 / 40 000 = 1 677.7 -> 1 677 = 104 x 16 + 13 -> 1 664
    An anoperms key replaces the expression, not the two caps."""
    cost = 2 * S if entry == "anosim" else 16 * max(S, C)
    assert BATCH_BYTES == 2 ** 26
    for n_lab in (1, 17, batch - 1, batch, batch + 1, 1000001, 1 << 21):
        for key in (0, 1, 17, batch + 5, PERMS_MAX, PERMS_MAX + 16):
            got = prog("plan", S, n_lab, cost, key)
            want = min(key if key > 0 else batch, PERMS_MAX, n_lab)
            groups = -(-want // PB)
            assert got == {"batch": want, "groups_max": groups, "stage_words": groups * S * PB}, (entry, S, C, n_lab, key)
