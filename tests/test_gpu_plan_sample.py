"""The pair kernel's launch plan is chosen from a SAMPLE of the columns (matrix_tied: the statistics of columns 0 .. 63 read
back -- of the first upload chunk only on the pipelined host path): the kernel family for 15 200 .. 30 656 rows, pairs per
wave for long columns, and the size of a pair's counter table (plan_k1 from the sample's largest tie-group count).  The
kernel stays correct on a column the sample did not see through its per-column joint-tie mode: list mode, count mode while
the column's tie groups have a counter each, row mode beyond.  Here the sample misrepresents the matrix on purpose:

  A. a continuous sample before tied columns, and a tied sample whose table the later columns straddle (cap - 1, cap,
     cap + 1 and 2 cap tie groups, list-mode columns, a continuous one, more than 4 094 groups) -- every entry (host
     all-pairs pipelined and not, a list of columns >= 64 only, the device-resident run and its REUSE_COUNTS perspective,
     the one-call matrix against the host assembly, two ranks on one device) bit for bit against each other and against
     row mode forced, a seeded pair subset against the oracle, and the columns permuted so that the tied ones are sampled;
  B. count mode at the limits of its 16-bit records: joint cells of up to 65 000 rows, two ~32 000-row groups in the two
     halves of one counter dword, the fill group as the big cell; flags 0 and EXACT_INT64.

Each case proves from the plan's verbose lines (stderr) that it reached the regime it was built for."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ATOL = 1e-10
NA_BITS = np.uint64(0x7FF00000000007A2)
S = 128
SAMPLE = 64

# Lengths, one per regime the sample decides, and what the plan must make of them (S = 128 columns: 8 128 pairs).
#   hint: largest tie-group count of the tied sample; cap: the table plan_k1 sizes to it (the smallest table >= hint it
#   allows; without the sample's hint the table would be smaller: 768 / 256 / 768 counters)
REGIMES = {
    17000: dict(hint=900, cap=1024, big=(40, 320), cont="whole-wave kernels", tied="half-wave kernels"),    # 9 words per lane
    24000: dict(hint=450, cap=512, big=(50, 330), cont="whole-wave kernels", tied="half-wave kernels"),     # 13 words per lane
    50000: dict(hint=900, cap=1024, big=(80, 400), cont="two pairs per wave", tied="one pair per wave"),    # long columns
}


def _oracle():
    from oracle import oracle as O
    return O


def _ntg(x):
    """Tie groups of >= 2 rows (no missing values here: no fill group)."""
    _v, c = np.unique(x[~np.isnan(x)], return_counts=True)
    return int((c >= 2).sum())


def _grouped(rng, n, sizes, perm=None):
    """A column whose tie groups have exactly the given sizes (each >= 2), laid out along the row permutation `perm`; every
    other row has a value of its own.  Values are distinct integers in random order."""
    sizes = np.asarray(sizes, dtype=np.int64)
    assert sizes.min(initial=2) >= 2 and sizes.sum() <= n
    vals = rng.permutation(n).astype(np.float64)
    lab = np.concatenate([np.repeat(np.arange(len(sizes)), sizes), len(sizes) + np.arange(n - int(sizes.sum()))])
    x = np.empty(n)
    x[rng.permutation(n) if perm is None else perm] = vals[lab]
    assert _ntg(x) == len(sizes)
    return x


def _count_like(rng, n):
    return rng.negative_binomial(2, 2.0 / 302.0, n).astype(np.float64)   # ~1 000 tie groups, most of many rows


def _matrix_cont_sample(n, seed):
    """Layout 1: columns 0 .. 63 continuous with sparse missing values; the rest count-like or of n / 10 distinct values."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, S))
    X[:, :SAMPLE][rng.random((n, SAMPLE)) < 0.01] = np.nan
    for c in range(SAMPLE, S):
        X[:, c] = _count_like(rng, n) if c % 2 == 0 else rng.integers(0, n // 10, n).astype(np.float64)
    X[:, S - 1][rng.random(n) < 0.05] = np.nan
    return np.asfortranarray(X), []


def _matrix_tied_sample(n, seed):
    """Layout 2: columns 0 .. 63 of `hint` - (c % 5) tie groups, a few dozen of them of >= 256 rows (a tied pair's group is
    long: the table is worth its waves); columns 64 .. built around the table that sample sizes."""
    R = REGIMES[n]
    rng = np.random.default_rng(seed)
    X = np.empty((n, S))
    nbig, bigsz = R["big"]
    for c in range(SAMPLE):
        g = R["hint"] - c % 5
        X[:, c] = _grouped(rng, n, [bigsz + int(rng.integers(0, 8))] * nbig + [2] * (g - nbig))
    cap = R["cap"]
    perm = rng.permutation(n)
    layout = 2 + rng.integers(0, 3, 2 * cap)        # group sizes 2 .. 4 shared by the columns on `perm`: their cells nest
    around = []
    for g in (cap - 1, cap, cap + 1, 2 * cap):      # on one row layout (joint cells are whole groups) and on its own
        around += [_grouped(rng, n, layout[:g], perm), _grouped(rng, n, 2 + rng.integers(0, 3, g))]
    around.append(_grouped(rng, n, [n // 100] * 100))                                   # list mode (<= 128 groups)
    around.append(_grouped(rng, n, [n // 120] * 120, perm))
    around.append(rng.standard_normal(n))                                               # continuous
    around.append(_grouped(rng, n, [2] * 4100))                                         # beyond the largest table
    cols = list(range(SAMPLE, SAMPLE + len(around)))
    for k, c in enumerate(cols):
        X[:, c] = around[k]
    for c in range(SAMPLE + len(around), S):
        X[:, c] = _count_like(rng, n) if c % 2 == 0 else rng.integers(0, n // 10, n).astype(np.float64)
    assert [_ntg(X[:, c]) for c in cols] == [cap - 1, cap - 1, cap, cap, cap + 1, cap + 1, 2 * cap, 2 * cap, 100, 120, 0, 4100]
    return np.asfortranarray(X), cols


def _pidx(i, j):
    return i * (2 * S - i - 1) // 2 + (j - i - 1)


def _same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y, equal_nan=True), f"{what}: output {k} differs ({int((x != y).sum())} entries)"
        if k == 0:
            assert np.array_equal(x.view(np.uint64)[np.isnan(x)], y.view(np.uint64)[np.isnan(y)]), f"{what}: NaN payloads"


def _oracle_subset(res, X, pairs, perspective):
    O = _oracle()
    out, cnt, rsn = res
    pi = np.array([p[0] for p in pairs], dtype=np.int32)
    pj = np.array([p[1] for p in pairs], dtype=np.int32)
    idx = _pidx(pi.astype(np.int64), pj.astype(np.int64))
    ref, rcnt, rrsn = O.ici_pairs(X, pi, pj, perspective)
    assert np.array_equal(rsn[idx], rrsn)
    ok = rrsn == 0
    assert np.array_equal(cnt[idx][ok], rcnt[ok][:, :cnt.shape[1]]), \
        [(int(pi[w]), int(pj[w])) for w in np.nonzero(np.any(cnt[idx] != rcnt[:, :cnt.shape[1]], axis=1) & ok)[0][:10]]
    assert np.array_equal(np.isnan(out[idx]), np.isnan(ref))
    if np.any(~np.isnan(ref)):
        assert float(np.nanmax(np.abs(out[idx] - ref))) <= ATOL
    na = np.isnan(out[idx][:, 0]) & (rrsn != 0)
    assert np.all(out[idx][na].view(np.uint64) == NA_BITS)


def _lines(err, key):
    return [ln for ln in err.splitlines() if key in ln]


def _readback(err):
    """(columns read back, largest tie-group count, verdict) of the one read-back line of a call."""
    ls = _lines(err, "columns read back")
    assert len(ls) == 1, err
    m = re.search(r"\] (\d+) columns read back: .*\(at most (\d+)\).* -> (.*)$", ls[0])
    assert m, ls[0]
    return int(m.group(1)), int(m.group(2)), m.group(3).strip()


def _k1(err):
    """[(np, half_items, tie-group counters)] of the K1 plan lines of a call."""
    out = []
    for ln in _lines(err, "K1 plan"):
        m = re.search(r"np=(\d+) half_items=(\d+) .*, (\d+) tie-group counters", ln)
        assert m, ln
        out.append(tuple(int(v) for v in m.groups()))
    assert out, err
    return out


@pytest.mark.parametrize("n", sorted(REGIMES))
@pytest.mark.parametrize("layout", ["cont_sample", "tied_sample"])
def test_plan_from_a_sample_that_misrepresents_the_matrix(plan_ctx, capfd, n, layout):
    import torch
    from icikendalltau_amd import _lib
    from tests.test_gpu_matrix import KEYS, _host_path

    R = REGIMES[n]
    X, around = (_matrix_cont_sample if layout == "cont_sample" else _matrix_tied_sample)(n, n + len(layout))
    P = S * (S - 1) // 2
    ctx = plan_ctx
    capfd.readouterr()

    def run(plan, *a, **kw):
        ctx.debug_set_plan(dict(plan or {}, verbose="1"))
        res = ctx.pairs(X, *a, **kw)
        return res, capfd.readouterr().err

    # --- the host entry, pipelined by chunks: the sample is the first chunk's columns ----------------------------------------
    base, err = run({"pipe": "1"})
    m, most, verdict = _readback(err)
    assert m < SAMPLE and "pipelined" in err, err
    plans = _k1(err)
    if layout == "cont_sample":
        assert most < 8 and verdict == R["cont"], err
        assert all(p[1] == 0 for p in plans), err                   # the whole-wave kernels for every column
        if n > 30656:
            assert all(p[0] == 2 for p in plans), err
    else:
        assert most == R["hint"] and verdict == R["tied"], err
        assert all(p[2] == R["cap"] for p in plans), err             # the table the sample asks for
    # --- not pipelined: the sample is columns 0 .. 63 -------------------------------------------------------------------------
    res, err = run({"pipe": "0"})
    m, most0, verdict0 = _readback(err)
    assert m == SAMPLE and verdict0 == verdict and _k1(err) == plans[:1], err
    _same(res, base, "pipe 0")
    # --- row mode for every column: the joint ties of every tie group row by row --------------------------------------------
    res, err = run({"tgmax": "-1"})
    assert all(p[2] == 0 for p in _k1(err)), err
    _same(res, base, "row mode")
    # --- a pair list of columns >= 64 only (the sample is still columns 0 .. 63) ---------------------------------------------
    qi, qj = (a + SAMPLE for a in np.triu_indices(S - SAMPLE, k=1))
    res, err = run(None, qi.astype(np.int32), qj.astype(np.int32))
    assert _readback(err)[1:] == (most0, verdict0), err
    _same(res, tuple(a[_pidx(qi, qj)] for a in base), "list of columns >= 64")
    # --- device-resident: prepare_dev + set_pairs_combn + run_dev, then the other perspective from the same counts -----------
    local, _err = run(None, perspective="local")
    ctx.debug_set_plan({"verbose": "1"})
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    dout = torch.empty((P, 4), dtype=torch.float64, device="cuda")
    dcnt = torch.zeros((P, len(_lib.CNT_FIELDS)), dtype=torch.int64, device="cuda")
    drsn = torch.zeros(P, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.prepare_dev(dX.data_ptr(), n, S, n)
    ctx.set_pairs_combn(S, 0, P)
    ctx.run_dev(1, 0, False, 0, dout.data_ptr(), dcnt.data_ptr(), drsn.data_ptr())
    ctx.sync()
    _same((dout.cpu().numpy(), dcnt.cpu().numpy(), drsn.cpu().numpy()), base, "device-resident")
    ctx.run_dev(0, 0, False, _lib.FLAG_REUSE_COUNTS, dout.data_ptr(), dcnt.data_ptr(), drsn.data_ptr())
    ctx.sync()
    _same((dout.cpu().numpy(), dcnt.cpu().numpy(), drsn.cpu().numpy()), local, "device-resident, REUSE_COUNTS local")
    assert _readback(capfd.readouterr().err)[1:] == (most0, verdict0)
    del dX, dout, dcnt, drsn
    # --- two ranks on one device (copies in place of the collectives) -----------------------------------------------------
    mc = _lib.MultiContext([0, 0], exchange="copy")
    try:
        _same(mc.pairs(X, perspective="global"), base, "two ranks")
        assert mc.ranks_used == 2
    finally:
        mc.close()
    # --- the one-call matrix entry against the host assembly of the pair results ---------------------------------------------
    from icikendalltau_amd import api
    names = [f"c{i}" for i in range(S)]
    fast = api.ici_kendalltau(X, global_na=(float("nan"),), colnames=names, engine=api.HipEngine())
    host = _host_path(X, names, global_na=(float("nan"),))
    for k in KEYS:
        assert np.array_equal(np.asarray(fast[k]), np.asarray(host[k]), equal_nan=True), k
    # --- the oracle on a seeded subset: the columns around the table among themselves and with three sampled columns, and
    #     pairs at random ----------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(n)
    pairs = [(a, b) for k, a in enumerate(around) for b in around[k + 1:]]
    pairs += [(s, a) for a in around for s in (0, 5, 37)]
    iu, ju = np.triu_indices(S, k=1)
    sel = rng.choice(len(iu), 300 if n < 30000 else 160, replace=False)
    pairs += [(int(iu[k]), int(ju[k])) for k in sel]
    if layout == "cont_sample":
        pairs += [(int(a), int(b)) for a, b in zip(rng.integers(0, SAMPLE, 40), rng.integers(SAMPLE, S, 40))]
    _oracle_subset(base, X, pairs, "global")
    _oracle_subset(local, X, pairs[:60] + pairs[-40:], "local")
    # --- metamorphic: the tied columns first, so that they are the sample; every pair's result maps through the permutation --
    order = np.concatenate([np.arange(SAMPLE, S), np.arange(SAMPLE)])
    inv = np.argsort(order)
    Xp = np.asfortranarray(X[:, order])
    ctx.debug_set_plan({"verbose": "1"})
    capfd.readouterr()
    res = ctx.pairs(Xp, inv[iu].astype(np.int32), inv[ju].astype(np.int32))     # (each pair in its first orientation)
    err = capfd.readouterr().err
    _m, most2, _verdict = _readback(err)
    assert most2 != most0, err                                            # another sample, another plan
    _same(res, base, "columns permuted")


# ---------------------------------------------------------------------------------------------------------------------------
# B. count mode at the limits of its 16-bit records
# ---------------------------------------------------------------------------------------------------------------------------
def _big_cell_matrix(n, ngroups, seed):
    """0: `ngroups` tie groups of two rows and one group of the rest; 1: equal to column 0 on the big group (a joint cell of
    n - 2 ngroups rows), its pairs of rows shuffled; 2 / 3: two groups of ~n / 2 - ngroups rows at adjacent values --
    adjacent tie-group indices, an even one and the next in one of the two columns -- beside the pairs; 4: column 2's big
    groups again (joint cells of ~n / 2 rows in both halves of one counter dword); 5 / 6: missing on the rows of column 0's
    big group (in the global perspective the fill group is the big cell); 7: continuous."""
    rng = np.random.default_rng(seed)
    X = np.empty((n, 8))
    pair_rows = rng.permutation(n)[: 2 * ngroups]
    rest = np.setdiff1d(np.arange(n), pair_rows)
    X[rest, 0] = 0.0
    X[pair_rows, 0] = np.repeat(np.arange(1, ngroups + 1, dtype=np.float64), 2)
    X[:, 1] = X[:, 0]
    X[pair_rows, 1] = rng.permutation(X[pair_rows, 1])
    half = rng.permutation(rest)
    h2 = len(half) // 2
    for c, shift in ((2, 0.0), (3, -1.0)):
        X[half[:h2], c] = 1.0
        X[half[h2:], c] = 2.0
        X[pair_rows, c] = np.repeat(np.arange(3, ngroups + 3, dtype=np.float64), 2)
        if shift:                                 # one pair group BELOW the two big ones: their indices move by one
            X[pair_rows[:2], c] = shift
    X[:, 4] = np.where(np.isin(np.arange(n), pair_rows), rng.standard_normal(n), X[:, 2])
    X[:, 5] = np.where(X[:, 0] == 0.0, np.nan, X[:, 0])
    X[:, 6] = np.where(X[:, 0] == 0.0, np.nan, rng.standard_normal(n))
    X[:, 7] = rng.standard_normal(n)
    for c in (0, 1, 2, 3):
        assert _ntg(X[:, c]) == ngroups + (1 if c < 2 else 2)
    return np.asfortranarray(X)


# both orientations of every pair: each column streams and is gathered
B_PAIRS = [(0, 1), (1, 0), (2, 4), (4, 2), (3, 4), (4, 3), (2, 3), (0, 2), (5, 6), (6, 5), (5, 1), (0, 7), (7, 3)]


@pytest.mark.parametrize("n,ngroups,base_plan", [(65535, 160, {}), (30656, 300, {"half": "1"}), (18336, 300, {"half": "1"})])
def test_count_mode_at_its_16_bit_limits(plan_ctx, capfd, n, ngroups, base_plan):
    O = _oracle()
    X = _big_cell_matrix(n, ngroups, n)
    pi = np.array([p[0] for p in B_PAIRS], dtype=np.int32)
    pj = np.array([p[1] for p in B_PAIRS], dtype=np.int32)
    whole = n > 30656
    refs = {}
    for flags in (0, 1):
        for persp in ("global", "local"):
            refs[flags, persp] = O.ici_pairs(X, pi, pj, persp, int32_compat=not flags)
    cell = int(((X[:, 0] == 0.0) & (X[:, 1] == 0.0)).sum())                  # the joint cell of columns 0 and 1
    assert cell > (46342 if whole else n - 2 * ngroups - 1)                       # (> 46 342: the reference's int32 wraps)
    capfd.readouterr()
    results = {}
    for plan in ({}, {"list": "0"}, {"tgmax": "1000000"}, {"np": "1"} if whole else {"split": "1"}, {"tgmax": "-1"}):
        plan_ctx.debug_set_plan(dict(base_plan, **plan, verbose="1"))
        for flags in (0, 1):
            for persp in ("global", "local"):
                out, cnt, rsn = plan_ctx.pairs(X, pi, pj, persp, flags=flags)
                err = capfd.readouterr().err
                k1 = _k1(err)
                if plan.get("tgmax") == "-1":
                    assert all(p[2] == 0 for p in k1), err
                else:          # a counter for every tie group of the gathered columns of `ngroups` + 1 / + 2 tie groups
                    assert all(p[2] >= ngroups + 2 for p in k1), err
                assert all((p[1] == 0) == whole for p in k1), err      # the kernel family the case was built for
                ref, rcnt, rrsn = refs[flags, persp]
                assert np.array_equal(rsn, rrsn), (plan, flags, persp)
                ok = rrsn == 0
                bad = np.nonzero(np.any(cnt != rcnt[:, :cnt.shape[1]], axis=1) & ok)[0]
                assert len(bad) == 0, (plan, flags, persp, [B_PAIRS[b] for b in bad], cnt[bad[0]], rcnt[bad[0]])
                assert np.array_equal(np.isnan(out), np.isnan(ref))
                assert float(np.nanmax(np.abs(out - ref))) <= ATOL, (plan, flags, persp)
                first = results.setdefault((flags, persp), (out, cnt, rsn))
                _same((out, cnt, rsn), first, f"plan {plan}")
