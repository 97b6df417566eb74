"""The typed, strided view of the caller's matrix (icikt_input) on the MI355X: k_ingest alone through
Context.convert_dev, every *_in entry against its _f64 twin on np.asfortranarray(X, dtype=float64), the front ends on a
C-ordered float32 matrix, and the argument errors.

The twin is the reference everywhere: the device matrix a view leaves behind is the float64 matrix the twin uploads, bit
for bit, and nothing behind it differs, so every output -- integers and doubles -- is compared for equality (NaN equal
to NaN).  cor_fast included: its kernels hold no floating-point atomics, and two calls of the _f64 entry on one input
agree bit for bit (test_cor_pairs_f64_is_bit_reproducible asserts that premise)."""
import ctypes

import numpy as np
import pytest

from icikendalltau_amd import _lib

pytestmark = pytest.mark.gpu

NP_DTYPES = {_lib.DTYPE_F64: np.float64, _lib.DTYPE_F32: np.float32, _lib.DTYPE_I32: np.int32, _lib.DTYPE_I64: np.int64}
NA_REAL_BITS = 0x7FF00000000007A2
SENTINEL = -12345.678
GNA = (np.nan, np.inf, 0)


# ---- the kernel alone ----------------------------------------------------------------------------------------------

def special_values(code):
    if code == _lib.DTYPE_F64:
        bits = [NA_REAL_BITS, 0x7FF8000000000000, 0xFFF8000000000BAD, 0x7FF0000000000000, 0xFFF0000000000000,
                0x8000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF]
        return np.array(bits, dtype=np.uint64).view(np.float64)
    if code == _lib.DTYPE_F32:
        bits = [0x7FC00000, 0xFFC00123, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000,
                0x007FFFFF, 0x00000001, 0x807FFFFF, 0x7F7FFFFF]     # NaNs, +-Inf, -0, largest / smallest subnormal, max
        return np.array(bits, dtype=np.uint32).view(np.float32)
    if code == _lib.DTYPE_I32:
        return np.array([-2**31, 2**31 - 1, 0, -1, 16777217], dtype=np.int32)
    return np.array([2**53 + 1, -(2**53 + 1), -2**63, 2**63 - 1, 2**53 + 3, 2**62 + 1, 0, -1], dtype=np.int64)


def source_block(rng, code, order, n, S, pad):
    """(buf, X): buf is the memory block as it lies (major x ld, the padding filled too), X the n x S view of it"""
    dt = NP_DTYPES[code]
    major, minor = (n, S) if order == _lib.ORDER_ROW else (S, n)
    if code in (_lib.DTYPE_F64, _lib.DTYPE_F32):
        buf = rng.standard_normal((major, minor + pad)).astype(dt)
    else:
        buf = rng.integers(-10**6, 10**6, size=(major, minor + pad)).astype(dt)
    X = buf[:, :minor] if order == _lib.ORDER_ROW else buf[:, :minor].T
    sp = special_values(code)
    k = min(sp.size, n * S)
    rr, cc = np.unravel_index(rng.permutation(n * S)[:k], (n, S))
    X[rr, cc] = sp[:k]
    return buf, X


def check_convert(ctx, rng, code, order, n, S, pad, dst_pad):
    import torch
    buf, X = source_block(rng, code, order, n, S, pad)
    ld = buf.shape[1]
    want = np.asfortranarray(X.astype(np.float64))
    d_src = torch.from_numpy(buf).cuda()
    dst_ld = n + dst_pad
    d_dst = torch.full((S, dst_ld), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                       # (the fill runs on torch's stream, the conversion on the context's)
    ctx.convert_dev(d_src.data_ptr(), code, order, n, S, ld, d_dst.data_ptr(), dst_ld)
    ctx.sync()
    got = d_dst.cpu().numpy()                      # row j = column j of the device matrix
    label = (code, order, n, S, pad, dst_pad)
    assert np.all(got[:, n:] == SENTINEL), label   # rows [n, dst_ld) of every column are untouched
    g, w = got[:, :n].T, want
    if code == _lib.DTYPE_F32:
        nan = np.isnan(X)
        assert np.array_equal(np.isnan(g), nan), label
        assert np.array_equal(g[~nan].view(np.uint64), w[~nan].view(np.uint64)), label
    else:
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(w).view(np.uint64)), label


SHAPES = [(1, 1), (1, 200), (200, 1), (63, 65), (64, 64), (65, 63), (129, 130)]


@pytest.mark.parametrize("order", [_lib.ORDER_COL, _lib.ORDER_ROW])
@pytest.mark.parametrize("code", sorted(NP_DTYPES))
def test_convert_dev_shapes_and_values(hip_ctx, code, order):
    rng = np.random.default_rng(100 * code + order)
    for n, S in SHAPES:
        for pad in (0, 3):
            check_convert(hip_ctx, rng, code, order, n, S, pad, dst_pad=pad)


@pytest.mark.parametrize("order", [_lib.ORDER_COL, _lib.ORDER_ROW])
@pytest.mark.parametrize("code", sorted(NP_DTYPES))
@pytest.mark.parametrize("n,S", [(3, 70000), (262144, 3)])
def test_convert_dev_past_the_grid_cap(hip_ctx, n, S, code, order):
    """More tiles than a launch has workgroups (1 024: icikt_ingest.hip; a ROW tile is 64 x 64 cells, a COL tile 512 rows
    of a column), so workgroups take a second round; no grid dimension grows with the matrix."""
    tiles = (-(-n // 64)) * (-(-S // 64)) if order == _lib.ORDER_ROW else (-(-n // 512)) * S
    assert tiles > 1024
    check_convert(hip_ctx, np.random.default_rng(n + code), code, order, n, S, pad=3, dst_pad=2)


def test_convert_dev_feeds_prepare_dev(hip_ctx):
    """The result is what icikt_prepare_dev takes: pairs from a device-resident float32 row-major tensor equal the host
    entry's on the same values."""
    import torch
    rng = np.random.default_rng(9)
    n, S = 300, 6
    X = rng.integers(0, 30, size=(n, S)).astype(np.float32)
    X[rng.random((n, S)) < 0.1] = np.nan
    d_src = torch.from_numpy(X).cuda()
    d_X = torch.empty((S, n), dtype=torch.float64, device="cuda")
    d_out = torch.empty((S * (S - 1) // 2, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hip_ctx.convert_dev(d_src.data_ptr(), _lib.DTYPE_F32, _lib.ORDER_ROW, n, S, S, d_X.data_ptr(), n)
    hip_ctx.prepare_dev(d_X.data_ptr(), n, S, n)
    hip_ctx.set_pairs_combn(S, 0, S * (S - 1) // 2)
    hip_ctx.run_dev(1, 0, False, 0, d_out.data_ptr())
    hip_ctx.sync()
    ref, _c, _r = hip_ctx.pairs(X, perspective="global", want_counts=False)
    assert np.array_equal(d_out.cpu().numpy(), ref, equal_nan=True)


# ---- every *_in entry against its _f64 twin ---------------------------------------------------------------------------

def base_matrices(n, S):
    """(M_float, M_int): quantised values float32 and int32 hold exactly, with ties; 8 % NaN, zeros and a few Inf in the
    float one, 8 % zeros in the integer one"""
    rng = np.random.default_rng(7 * n + S)
    q = rng.integers(1, 60, size=(n, S))
    Mf = q * 0.25
    Mf[rng.random((n, S)) < 0.08] = np.nan
    Mf[rng.random((n, S)) < 0.03] = 0.0
    Mf[rng.random((n, S)) < 0.002] = np.inf
    Mi = q.copy()
    Mi[rng.random((n, S)) < 0.08] = 0
    return np.asfortranarray(Mf), np.asfortranarray(Mi.astype(np.float64))


def inputs_of(Mf, Mi):
    n, S = Mf.shape
    parent = np.full((n, S + 5), 99.0)
    parent[:, 2:2 + S] = Mf
    return {
        "C float64": ("f", np.ascontiguousarray(Mf)),
        "C float32": ("f", np.ascontiguousarray(Mf.astype(np.float32))),
        "C int32": ("i", np.ascontiguousarray(Mi.astype(np.int32))),
        "F float32": ("f", np.asfortranarray(Mf.astype(np.float32))),
        "F int64": ("i", np.asfortranarray(Mi.astype(np.int64))),
        "row-major slice, ld > n_samp": ("f", parent[:, 2:2 + S]),
    }


def run_entries(ctx, X, S, big):
    """every host entry once: {name: tuple of outputs}"""
    rng = np.random.default_rng(S)
    P = 40 if big else S * (S - 1) // 2
    pi = rng.integers(0, S, size=P).astype(np.int32)
    pj = ((pi + 1 + rng.integers(0, S - 1, size=P)) % S).astype(np.int32)      # (no self pairs)
    cls = (np.arange(S) % 3).astype(np.int32)
    out = {}
    out["pairs"] = ctx.pairs(X, perspective="global")
    out["pairs list"] = ctx.pairs(X, pi, pj, perspective="local", want_counts=False)
    out["matrix"] = ctx.matrix(X, global_na=GNA)
    out["pairs_complete"] = ctx.pairs_complete(X, pi, pj, want_counts=True)
    out["missingness"] = (ctx.missingness(X, pi, pj),)
    out["cor pearson pairwise"] = ctx.cor_pairs(X, pi, pj, "pearson", pairwise=True)
    out["cor spearman pairwise"] = ctx.cor_pairs(X, pi, pj, "spearman", pairwise=True)
    out["col_medians"] = (ctx.col_medians(X, na_rm=True, global_na=GNA), ctx.col_medians(X, na_rm=False))
    out["censor_counts"] = ctx.censor_counts(X, GNA, cls, 3, want_medians=True)
    for label, cols in (("consecutive", np.arange(2, min(S, 40), dtype=np.int32)),
                        ("gathered", np.array([5, 0, 3, 6][:S], dtype=np.int32))):
        r = ctx.rank_order(X, GNA, cols)
        out["rank_order " + label] = tuple(r[k] for k in sorted(r))
    return out


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (int, np.integer)):
        return int(a) == int(b)
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))
    return np.array_equal(a, b)


def assert_same_outputs(got, ref, label):
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert len(got[name]) == len(ref[name]), (label, name)
        for k, (g, r) in enumerate(zip(got[name], ref[name])):
            assert same(g, r), (label, name, k)


@pytest.fixture(scope="module")
def twin_refs(hip_ctx):
    """The _f64 entries' outputs on the float and the integer base matrix of a shape, computed once"""
    cache = {}

    def get(n, S):
        if (n, S) not in cache:
            Mf, Mi = base_matrices(n, S)
            hip_ctx.f64_entries = True
            try:
                cache[(n, S)] = (Mf, Mi, {"f": run_entries(hip_ctx, Mf, S, n > 1000),
                                          "i": run_entries(hip_ctx, Mi, S, n > 1000)})
            finally:
                hip_ctx.f64_entries = False
        return cache[(n, S)]
    return get


INPUTS = ["C float64", "C float32", "C int32", "F float32", "F int64", "row-major slice, ld > n_samp"]


@pytest.mark.parametrize("which", INPUTS)
@pytest.mark.parametrize("n,S", [(50, 7), (4000, 600)])
def test_in_entries_equal_their_f64_twins(hip_ctx, twin_refs, n, S, which):
    """50 x 7 is below 256 KB (the runtime's own staging path); 4 000 x 600 is 19 MB in float64: staged through the
    library's pinned buffer in three chunks."""
    Mf, Mi, refs = twin_refs(n, S)
    kind, X = inputs_of(Mf, Mi)[which]
    a, _code, _order, _ld, copied = _lib.input_view(X)
    assert copied is False and a is X
    assert np.array_equal(np.asfortranarray(X, dtype=np.float64), Mf if kind == "f" else Mi, equal_nan=True)
    assert_same_outputs(run_entries(hip_ctx, X, S, n > 1000), refs[kind], which)


@pytest.mark.parametrize("which", ["C float32", "C int32", "F float32", "row-major slice, ld > n_samp"])
@pytest.mark.parametrize("pipe", [0, 1])
def test_pairs_in_with_and_without_the_chunk_pipeline(plan_ctx, twin_refs, which, pipe):
    n, S = 4000, 600
    Mf, Mi, refs = twin_refs(n, S)
    kind, X = inputs_of(Mf, Mi)[which]
    plan_ctx.debug_set_plan(f"pipe={pipe}")
    got = plan_ctx.pairs(X, perspective="global")
    for k, (g, r) in enumerate(zip(got, refs[kind]["pairs"])):
        assert same(g, r), (which, pipe, k)
    out5 = plan_ctx.matrix(X, global_na=GNA)
    for k, (g, r) in enumerate(zip(out5, refs[kind]["matrix"])):
        assert same(g, r), (which, pipe, "matrix", k)


def test_pairs_in_from_caller_pinned_row_major_memory(hip_ctx, twin_refs):
    n, S = 4000, 600
    Mf, _Mi, refs = twin_refs(n, S)
    Xp = _lib.pinned_empty((n, S), dtype=np.float32, order="C")
    Xp[...] = Mf
    assert _lib.input_view(Xp)[1:] == (_lib.DTYPE_F32, _lib.ORDER_ROW, S, False)
    got = hip_ctx.pairs(Xp, perspective="global", flags=_lib.FLAG_HOST_PINNED)
    for k, (g, r) in enumerate(zip(got, refs["f"]["pairs"])):
        assert same(g, r), k
    out5 = hip_ctx.matrix(Xp, global_na=GNA, flags=_lib.FLAG_HOST_PINNED)
    for k, (g, r) in enumerate(zip(out5, refs["f"]["matrix"])):
        assert same(g, r), ("matrix", k)


def test_cor_pairs_f64_is_bit_reproducible(hip_ctx, twin_refs):
    """The premise of comparing cor_fast's doubles for equality: two calls of the _f64 entry agree bit for bit."""
    n, S = 4000, 600
    Mf, _Mi, refs = twin_refs(n, S)
    hip_ctx.f64_entries = True
    try:
        again = run_entries(hip_ctx, Mf, S, True)
    finally:
        hip_ctx.f64_entries = False
    for name in ("cor pearson pairwise", "cor spearman pairwise"):
        for g, r in zip(again[name], refs["f"][name]):
            assert same(g, r), name


# ---- the front ends ----------------------------------------------------------------------------------------------------

def same_result(a, b, path=""):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            if k != "run_time":
                same_result(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            same_result(x, y, f"{path}[{k}]")
    elif hasattr(a, "to_numpy"):
        assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index), path
        for col in a.columns:
            same_result(a[col].to_numpy(), b[col].to_numpy(), f"{path}/{col}")
    elif isinstance(a, np.ndarray) and a.dtype.kind in "fiub":
        assert same(a, b), path
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and all(x == y for x, y in zip(a.ravel(), b.ravel())), path
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), path
    else:
        assert a == b, path


def test_front_ends_on_a_c_ordered_float32_matrix(hip_ctx):
    import warnings
    import icikendalltau_amd as pkg
    rng = np.random.default_rng(31)
    n, S = 300, 9
    X32 = (rng.integers(0, 50, size=(n, S)) * 0.5).astype(np.float32)
    X32[rng.random((n, S)) < 0.1] = np.nan
    assert X32.flags.c_contiguous and _lib.input_view(X32)[4] is False
    X64 = np.asfortranarray(X32, dtype=np.float64)
    names = [f"s{j}" for j in range(S)]
    classes = ["a", "b", "c"] * 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for label, call in (
                ("ici_kendalltau", lambda X: pkg.ici_kendalltau(X, colnames=names)),
                ("cor_fast", lambda X: pkg.cor_fast(X, use="pairwise.complete.obs", colnames=names)),
                ("test_left_censorship", lambda X: pkg.test_left_censorship(X, sample_classes=classes)),
                ("calculate_matrix_medians", lambda X: pkg.calculate_matrix_medians(X, na_rm=True)),
                ("calculate_matrix_medians rows", lambda X: pkg.calculate_matrix_medians(X, use="row", na_rm=True))):
            same_result(call(X32), call(X64), label)


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_in_entries_and_convert_dev_refuse_bad_views(hip_ctx):
    """dtype 7, order 2, ld = extent - 1 and null data: ICIKT_E_INVALID (-1) and a message, never a HIP error; nothing
    is written.  262 145 rows are refused as the _f64 entries refuse them."""
    import torch
    L, h = _lib.lib(), hip_ctx._h
    n, S = 60, 5
    P = S * (S - 1) // 2
    rng = np.random.default_rng(2)
    Xc = np.ascontiguousarray(rng.standard_normal((n, S)).astype(np.float32))
    Xf = np.asfortranarray(Xc)
    pi, pj = [a.astype(np.int32) for a in np.triu_indices(S, k=1)]
    cls = np.zeros(S, dtype=np.int32)
    cols = np.arange(S, dtype=np.int32)
    gna = np.array([np.nan, 0.0])
    o = {k: np.full(sz, 7.0) for k, sz in (("out4", (P, 4)), ("out5", (5, S, S)), ("out3", (P, 3)), ("med", S),
                                           ("medrank", n), ("orig", n * S), ("ordd", n * S))}
    oi = {k: np.full(sz, 7, dtype=dt) for k, sz, dt in (
        ("cnt", (P, 11), np.int64), ("rsn", P, np.int32), ("miss", P, np.int64), ("tr", 1, np.int64), ("su", 1, np.int64),
        ("ex", 1, np.int64), ("nk", 1, np.int64), ("nna", n, np.int32), ("rord", n, np.int32), ("cord", S, np.int32),
        ("keep", (S, n), np.uint8), ("rc5", 5, np.int64))}
    p = lambda a: a.ctypes.data                                            # noqa: E731

    def calls(v, nf=n):
        r = ctypes.byref(v)
        return {
            "pairs": lambda: L.icikt_pairs_in(h, r, nf, S, None, None, 0, 1, 0, 0, 0, p(o["out4"]), p(oi["cnt"]), p(oi["rsn"])),
            "matrix": lambda: L.icikt_matrix_in(h, r, nf, S, p(gna), 2, None, None, 0, 1, 0, 0, 0, 1, 1, p(o["out5"]),
                                                p(oi["keep"]), p(oi["rc5"])),
            "pairs_complete": lambda: L.icikt_pairs_complete_in(h, r, nf, S, p(pi), p(pj), P, 0, 0, 0, p(o["out4"]), None, None),
            "missingness": lambda: L.icikt_missingness_in(h, r, nf, S, p(pi), p(pj), P, p(oi["miss"])),
            "cor_pairs": lambda: L.icikt_cor_pairs_in(h, r, nf, S, p(pi), p(pj), P, 0, 1, 0, 0, 0, p(o["out3"]), p(oi["rsn"])),
            "col_medians": lambda: L.icikt_col_medians_in(h, r, nf, S, p(gna), 2, 1, 0, p(o["med"])),
            "censor_counts": lambda: L.icikt_censor_counts_in(h, r, nf, S, p(gna), 2, p(cls), 1, 0, p(oi["tr"]), p(oi["su"]),
                                                              p(oi["ex"]), p(o["med"])),
            "rank_order": lambda: L.icikt_rank_order_in(h, r, nf, S, p(gna), 2, p(cols), S, 0, p(oi["nk"]), p(oi["nna"]),
                                                        p(o["medrank"]), p(oi["rord"]), p(oi["cord"]), p(o["orig"]), p(o["ordd"])),
        }

    def untouched():
        return all(np.all(a == 7.0) for a in o.values()) and all(
            np.all(a == 7) for k, a in oi.items() if k not in ("tr", "su", "ex", "nk", "rc5"))

    V = _lib.InputView
    bad = {
        "dtype 7": V(p(Xc), 7, _lib.ORDER_ROW, S),
        "dtype -1": V(p(Xc), -1, _lib.ORDER_ROW, S),
        "order 2": V(p(Xc), _lib.DTYPE_F32, 2, S),
        "row-major ld = n_samp - 1": V(p(Xc), _lib.DTYPE_F32, _lib.ORDER_ROW, S - 1),
        "column-major ld = n_feat - 1": V(p(Xf), _lib.DTYPE_F32, _lib.ORDER_COL, n - 1),
        "null data": V(None, _lib.DTYPE_F32, _lib.ORDER_ROW, S),
    }
    tried = 0
    for what, v in bad.items():
        for name, call in calls(v).items():
            rc = call()
            assert rc == -1 and len(L.icikt_last_error(h)) > 0, (what, name, rc)
            assert untouched(), (what, name)
            tried += 1
    for name in calls(bad["dtype 7"]):                                   # a null view
        fn = getattr(L, f"icikt_{name}_in")
        args = [h, None, n, S] + [None] * (len(fn.argtypes) - 4)
        for k, t in enumerate(fn.argtypes):
            if t in (ctypes.c_int, ctypes.c_int64, ctypes.c_uint32):
                args[k] = 0 if k >= 4 else args[k]
        rc = fn(*args)
        assert rc == -1 and b"null" in L.icikt_last_error(h), (name, rc)
        tried += 1
    too_long = V(p(Xc), _lib.DTYPE_F32, _lib.ORDER_ROW, S)                  # (refused before a cell is read)
    for name, call in calls(too_long, nf=262145).items():
        rc = call()
        assert rc == -4 and b"262144" in L.icikt_last_error(h) and b"ICIKT_MAX_FEATURES" in L.icikt_last_error(h), (name, rc)
        assert untouched(), name
        tried += 1
    with pytest.raises(_lib.IciktError, match="262144"):
        hip_ctx.pairs(np.zeros((262145, 4), dtype=np.float32))
    # ---- icikt_convert_dev ---------------------------------------------------------------------------------------------
    d_src = torch.from_numpy(Xc).cuda()
    d_dst = torch.full((S, n), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for what, a in {
        "dtype 7": (d_src.data_ptr(), 7, 1, n, S, S, d_dst.data_ptr(), n),
        "order 2": (d_src.data_ptr(), 1, 2, n, S, S, d_dst.data_ptr(), n),
        "ld = n_samp - 1": (d_src.data_ptr(), 1, 1, n, S, S - 1, d_dst.data_ptr(), n),
        "ld = n_feat - 1": (d_src.data_ptr(), 1, 0, n, S, n - 1, d_dst.data_ptr(), n),
        "null source": (None, 1, 1, n, S, S, d_dst.data_ptr(), n),
        "null destination": (d_src.data_ptr(), 1, 1, n, S, S, None, n),
        "dst_ld = n_feat - 1": (d_src.data_ptr(), 1, 1, n, S, S, d_dst.data_ptr(), n - 1),
        "negative n_feat": (d_src.data_ptr(), 1, 1, -1, S, S, d_dst.data_ptr(), n),
    }.items():
        rc = L.icikt_convert_dev(h, *a)
        assert rc == -1 and len(L.icikt_last_error(h)) > 0, (what, rc)
        tried += 1
    assert L.icikt_convert_dev(h, d_src.data_ptr(), 1, 1, 262145, S, S, d_dst.data_ptr(), 262145) == -4
    assert L.icikt_convert_dev(None, d_src.data_ptr(), 1, 1, n, S, S, d_dst.data_ptr(), n) == -1
    hip_ctx.sync()
    assert torch.all(d_dst == 7.0)
    assert tried >= 6 * 8 + 8 + 8 + 8
    # and the context still computes
    got = hip_ctx.pairs(Xc, perspective="global", want_counts=False)[0]
    hip_ctx.f64_entries = True
    try:
        ref = hip_ctx.pairs(Xc, perspective="global", want_counts=False)[0]
    finally:
        hip_ctx.f64_entries = False
    assert np.array_equal(got, ref, equal_nan=True)
