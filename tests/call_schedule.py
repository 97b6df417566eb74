"""Inputs, call vocabulary and seeded call schedules for the tests of one context serving many calls
(tests/test_call_schedule_host.py checks the schedules, tests/test_gpu_call_order.py runs them).  Plain numpy: nothing
here touches a device; `run` only calls the methods of the context it is given.

A context keeps every device buffer it ever allocated and each entry resets its own piece of that state (DESIGN.md
section 16, "what a call finds in the context").  A schedule is a list of `Call`s over all entries of the library, on
data sets of five shapes, built so that every entry runs right after every other entry, after larger, smaller and other
data of the same shape, and after every kind of refused call: `violations` states the conditions and checks them.

How long a schedule is.  d_X / d_ingest / d_indptr are every entry's, so "every entry directly follows every other entry
that shares a buffer with it" asks for all 17 * 16 ordered pairs of entries: at least 273 calls, and an Euler circuit of
the complete digraph on the entries gives exactly that.  Each of the 3 kinds of refused call is followed by each of 9
entries: 27 refused calls and 27 calls behind them.  A schedule therefore has 327 calls; nearly all are tiny.
"""
from collections import namedtuple

import numpy as np

from icikendalltau_amd import _lib
from tests.anosim_checker import documented_permutations

# ---- data ------------------------------------------------------------------------------------------------------------

SHAPES = ((3, 40), (65, 700), (130, 40), (130, 16), (300, 40))      # (S, n)
# data key -> (S, n, kind, the form its matrix travels in where the entry has that form)
DATA = {
    "s3": (3, 40, "continuous", "f64"),
    "a65": (65, 700, "continuous", "csc"),
    "b65": (65, 700, "factor", "f32"),
    "a130": (130, 40, "continuous", "f64"),
    "b130": (130, 40, "factor", "f32"),
    "t130": (130, 16, "tied", "f32"),
    "a300": (300, 40, "continuous", "csc"),
}
TWIN = {"a65": "b65", "b65": "a65", "a130": "b130", "b130": "a130"}   # the other data set of the same shape
DUP = "dup130"        # a130 as CSC with one row index repeated in column 120: refused by the device-side check
BIG, SMALL = "a300", "s3"
_SEED = {"s3": 301, "a65": 302, "b65": 303, "a130": 304, "b130": 305, "t130": 306, "a300": 307}
GNA = (np.nan, np.inf, 0.0)                                         # the diagnostics' global_na
SPEC = "tkblock=1000,padjtile=33,anostrip=64,anoperms=16"           # the plan the schedules alternate with the library's
ALPHAS = (0.01, 0.05, 0.5)
PROBS = (0, 1, 0.5, 0.25, 1 / 3, 0.999, 0.5, 0.1)
BREAKS = np.linspace(-1.0, 1.0, 8)
N_PERM = 33
_cache = {}


def dense(key):
    """The float64 column-major matrix [n, S] of a data set: the values every form of it carries (a data set that
    travels as float32 holds float32 values)."""
    if key in _cache:
        return _cache[key]
    if key == DUP:
        X = dense("a130")
    else:
        S, n, kind, form = DATA[key]
        rng = np.random.default_rng(_SEED[key])
        if kind == "continuous":        # 8 % NaN, a constant column and an all-NaN column
            X = rng.standard_normal((n, S))
            X[rng.random((n, S)) < 0.08] = np.nan
            if S > 8:
                X[:, 5] = 1.0
                X[:, S - 2] = np.nan
        elif kind == "factor":          # one shared factor (tests/test_gpu_padjust._correlated), loadings in [0.7, 0.95)
            f = rng.standard_normal(n)
            load = rng.uniform(0.7, 0.95, S)
            X = f[:, None] * load[None, :] + rng.standard_normal((n, S)) * np.sqrt(1.0 - load ** 2)[None, :]
            X[rng.random((n, S)) < 0.08] = np.nan
        else:                           # few rows of small integers: long runs of equal tau, equal p
            X = rng.integers(0, 4, size=(n, S)).astype(np.float64)
            X[rng.random((n, S)) < 0.03] = np.nan
        if form == "f32":
            X = X.astype(np.float32).astype(np.float64)
        X = np.asfortranarray(X)
    X.setflags(write=False)
    _cache[key] = X
    return X


def n_samp(key):
    return 130 if key == DUP else DATA[key][0]


def _csc(X, dup_col=None):
    """X as CSC arrays: the cells that are not NaN are the entries, fill = NaN.  dup_col: that column's second entry
    repeats the row of its first."""
    n, S = X.shape
    have = ~np.isnan(X)
    rows, cols = np.nonzero(have.T)[1], np.nonzero(have.T)[0]       # column by column, rows ascending
    indptr = np.zeros(S + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(have.sum(axis=0))
    indices = rows.astype(np.int32)
    data = np.ascontiguousarray(X.T[have.T])
    assert np.array_equal(cols, np.repeat(np.arange(S), np.diff(indptr)))
    if dup_col is not None:
        p = int(indptr[dup_col])
        assert indptr[dup_col + 1] - p >= 2
        indices[p + 1] = indices[p]
    return _lib.CscView(data, indices, indptr, (n, S), np.nan, False)


CSC_ENTRIES = ("pairs", "matrix", "missingness", "col_medians", "censor_counts", "rank_order", "topk", "edges",
               "class_medians", "quantiles", "class_matrix", "padjust", "mst", "anosim")


def form_of(entry, key):
    """The form `entry` gets the data set in: its own where the entry has it, else column-major float64."""
    if entry == "pair":
        return "f64"
    if key == DUP:
        return "csc"
    form = DATA[key][3]
    return "f64" if form == "csc" and entry not in CSC_ENTRIES else form


def matrix_in(key, form):
    ck = (key, form)
    if ck not in _cache:
        X = dense(key)
        if form == "f64":
            _cache[ck] = X
        elif form == "f32":
            M = np.ascontiguousarray(X, dtype=np.float32)           # a C-contiguous float32 view: row-major
            assert M.flags.c_contiguous and np.array_equal(M.astype(np.float64), X, equal_nan=True)
            _cache[ck] = M
        else:
            _cache[ck] = _csc(X, dup_col=120 if key == DUP else None)
            if key != DUP:
                assert np.array_equal(_cache[ck].toarray(), X, equal_nan=True)
    return _cache[ck]


def pair_list(S):
    """up to 200 pairs i < j of the triangle, in a shuffled order"""
    iu, ju = np.triu_indices(S, k=1)
    sel = np.random.default_rng(S).permutation(iu.shape[0])[:200]
    return iu[sel].astype(np.int32), ju[sel].astype(np.int32)


def classes3(S):
    """three interleaved classes and a singleton"""
    cls = (np.arange(S) % 3).astype(np.int32)
    cls[S - 1] = 3
    return cls, 4


def classes5(S):
    """five classes of unequal size in shuffled order, class 3 a singleton (S = 3: three of the five are empty)"""
    cls = np.zeros(S, dtype=np.int32)
    cls[S // 3:] = 1
    cls[S // 2:] = 2
    cls[S - 1 - S // 5:S - 1] = 4
    cls[-1] = 3
    np.random.default_rng(4).shuffle(cls)
    return cls, 5


def labellings(S):
    cls, n_class = classes5(S)
    return cls, n_class, documented_permutations(cls, N_PERM, 7)


# ---- vocabulary ------------------------------------------------------------------------------------------------------

OTHER = ("pairs", "pair", "matrix", "pairs_complete", "missingness", "cor_pairs", "col_medians", "censor_counts",
         "rank_order")
SELECT = ("topk", "edges", "class_medians", "class_matrix", "quantiles", "padjust", "mst", "anosim")
ENTRIES = OTHER + SELECT
VARIANTS = {
    "pairs": ("all", "list"), "pair": ("xy",), "matrix": ("full",), "pairs_complete": ("list",),
    "missingness": ("list",), "cor_pairs": ("pearson", "spearman_pw"), "col_medians": ("na_rm",),
    "censor_counts": ("cls3",), "rank_order": ("every_other",),
    "topk": ("k1", "k7"), "edges": ("equal", "short"), "class_medians": ("one", "cls3"), "class_matrix": ("cls3",),
    "quantiles": ("full", "hist"), "padjust": ("BH", "holm"), "mst": ("all", "median"), "anosim": ("perm33",),
}
DETERMINISM = ("cor_pairs", "col_medians", "censor_counts", "rank_order")   # compared bitwise only if two fresh contexts agree
FOLLOWERS = SELECT + ("matrix",)             # what must directly follow every kind of refused call
FAIL_KINDS = ("a", "b", "c")                 # a: perspective = 7; b: a duplicate CSC entry; c: a bad label in the last labelling
FAIL_MESSAGE = {
    "a": r"code -1.*{who}: perspective must be local \(0\) or global \(1\)",
    "b": r"code -1.*duplicate entry \(sum_duplicates\)",
    "c": r"code -1.*anosim: perm_cls\[32\]\[\d+\] = 5 is outside 0 \.\. n_class - 1",
}
# the context's buffers (csrc/icikt_host.h) that more than one entry uses, and the entries that use them
BUFFER_USERS = {
    "d_X, d_ingest, d_indptr": ENTRIES,
    "d_out4, d_reasons": ("pairs", "pair", "matrix", "pairs_complete", "cor_pairs") + SELECT,
    "d_red": ("matrix",) + SELECT,
    "d_counts": ("pairs", "pair", "missingness"),
    "the sort's counts / agg": ("padjust", "anosim"),
    "colsort scratch": ("quantiles", "padjust"),
}

# one call: entry and variant name the method and its fixed arguments, data the data set, form how the matrix travels,
# plan the debug plan set before it (None: the library's choice), fail the kind of refusal it must end in (None: none)
Call = namedtuple("Call", "entry variant data form plan fail")


def ref_key(call):
    """What the answer of a successful call depends on (the plan keys change no answer)."""
    return (call.entry, call.variant, call.data, call.form)


def answer_key(call):
    """Two successful calls of one entry with the same answer_key give the same answer: the forms of a data set carry
    the same values."""
    return (call.entry, call.variant, call.data)


def run(ctx, call, resolve=None):
    """Run `call` on `ctx` and return its result as a flat tuple.  resolve(name, data, form): the two arguments that
    come out of the data's own matrix -- "n_edges" (the pairs with raw >= 0) and "median_raw"."""
    e, v, key = call.entry, call.variant, call.data
    S = n_samp(key)
    X = matrix_in(key, call.form)
    persp = 7 if call.fail == "a" else "global"
    if e == "pair":
        D = dense(key)
        out, cnt, rsn = ctx.pair(np.array(D[:, 0]), np.array(D[:, 1]), perspective="global")
        return (out, np.array(list(cnt.values()), dtype=np.int64), rsn)
    if e == "pairs":
        return ctx.pairs(X) if v == "all" else ctx.pairs(X, *pair_list(S))
    if e == "matrix":
        return ctx.matrix(X)
    if e == "pairs_complete":
        return ctx.pairs_complete(X, *pair_list(S), want_counts=True)
    if e == "missingness":
        return (ctx.missingness(X, *pair_list(S)),)
    if e == "cor_pairs":
        return ctx.cor_pairs(X, *pair_list(S), *(("pearson", False) if v == "pearson" else ("spearman", True)))
    if e == "col_medians":
        return (ctx.col_medians(X, True, global_na=GNA),)
    if e == "censor_counts":
        return ctx.censor_counts(X, GNA, (np.arange(S) % 3).astype(np.int32), 3, want_medians=True)
    if e == "rank_order":
        d = ctx.rank_order(X, GNA, np.arange(0, S, 2, dtype=np.int32))
        return tuple(d[k] for k in ("n_kept", "n_na", "median_rank", "row_order", "col_order", "original", "ordered"))
    total = S * (S - 1) // 2
    if e == "topk":
        return ctx.topk(X, 1 if v == "k1" else 7, perspective=persp)
    if e == "edges":
        m = total if call.fail else resolve("n_edges", key, call.form)
        return ctx.edges(X, min_raw=0.0, max_edges=m if v == "equal" else max(m // 3, 1), perspective=persp)
    if e == "class_medians":
        return ctx.class_medians(X, *(classes3(S) if v == "cls3" else ()), perspective=persp)
    if e == "class_matrix":
        return ctx.class_matrix(X, *classes3(S), perspective=persp)
    if e == "quantiles":
        if v == "hist":
            return ctx.quantiles(X, (), BREAKS, perspective=persp)
        return ctx.quantiles(X, PROBS, BREAKS, *classes3(S), perspective=persp)
    if e == "padjust":
        return ctx.padjust(X, v if v in ("BH", "holm") else "BH", ALPHAS, total, perspective=persp)
    if e == "mst":
        thr = None if (v == "all" or call.fail) else resolve("median_raw", key, call.form)
        return ctx.mst(X, min_raw=thr, perspective=persp)
    if e == "anosim":
        cls, n_class, perms = labellings(S)
        if call.fail == "c":
            perms = perms.copy()
            perms[N_PERM - 1, S // 2] = n_class
        return ctx.anosim(X, cls, n_class, perms, perspective=persp)
    raise ValueError(e)


# ---- schedules -------------------------------------------------------------------------------------------------------

SEEDS = (1, 2, 3, 4)


def _euler(rng):
    """An Euler circuit of the complete digraph on ENTRIES (Hierholzer over shuffled edge lists): every ordered pair of
    different entries is adjacent exactly once."""
    out = {e: [f for f in rng.permutation(ENTRIES) if f != e] for e in ENTRIES}
    stack, circuit = [str(rng.choice(ENTRIES))], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(str(out[v].pop()))
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == len(ENTRIES) * (len(ENTRIES) - 1) + 1
    return circuit


def _build(rng):
    ent = _euler(rng)
    n = len(ent)
    keys = list(DATA)
    data = [str(rng.choice(keys)) for _ in range(n)]
    forced, prevs = set(), set()
    # every selection entry directly after a larger, a smaller and the twin data set
    for e in SELECT:
        for cond in ("larger", "smaller", "twin"):
            spots = [i for i in range(1, n) if ent[i] == e and ent[i - 1] != "pair" and not {i - 1, i} & forced]
            i = int(rng.choice(spots))
            if cond == "larger":
                data[i - 1], data[i] = BIG, str(rng.choice([k for k in keys if k != BIG]))
            elif cond == "smaller":
                data[i - 1], data[i] = SMALL, str(rng.choice([k for k in keys if k != SMALL]))
            else:
                data[i] = str(rng.choice(sorted(TWIN)))
                data[i - 1] = TWIN[data[i]]
            forced |= {i - 1, i}
            prevs.add(i - 1)
    # a refused call of every kind directly before every follower: the pair goes in behind a call of the follower's
    # entry, so no adjacency of the circuit is lost
    insert = {}
    rot = {k: [str(x) for x in rng.permutation(SELECT)] for k in "ab"}
    for kind in FAIL_KINDS:
        for f in rng.permutation(FOLLOWERS):
            spots = [i for i in range(n) if ent[i] == f and i not in prevs and i not in insert]
            i = int(rng.choice(spots))
            who = "anosim" if kind == "c" else rot[kind][len([1 for v in insert.values() if v[0] == kind]) % len(SELECT)]
            insert[i] = (kind, who)
    slots = []                                   # (entry, data or None, fixed, fail kind)
    for i in range(n):
        slots.append((ent[i], data[i], i in forced, None))
        if i in insert:
            kind, who = insert[i]
            slots.append((who, {"a": "a130", "b": DUP, "c": str(rng.choice(keys))}[kind], True, kind))
            slots.append((ent[i], str(rng.choice(keys)), False, None))
    # variants in turn, the plans alternating; a call never repeats its entry's previous successful call
    calls, last, turn = [], {}, {e: int(rng.integers(0, 2)) for e in ENTRIES}
    phase = int(rng.integers(0, 2))
    for pos, (e, key, fixed, kind) in enumerate(slots):
        plan = SPEC if (kind in ("b", "c") or (pos + phase) % 2) else None
        if kind:
            calls.append(Call(e, VARIANTS[e][0], key, form_of(e, key), plan, kind))
            continue
        v = VARIANTS[e][turn[e] % len(VARIANTS[e])]
        turn[e] += 1
        if last.get(e) == (v, key) and not fixed:
            key = str(rng.choice([k for k in keys if k != key]))
        last[e] = (v, key)
        calls.append(Call(e, v, key, form_of(e, key), plan, None))
    return calls


def schedule(seed):
    """The schedule of a seed: deterministic, and free of violations by construction (a draw that is not is dropped)."""
    for attempt in range(200):
        calls = _build(np.random.default_rng([int(seed), attempt]))
        if not violations(calls):
            return calls
    raise AssertionError(f"no schedule for seed {seed}")


def hand_written():
    """The eight selection entries at 300, then 3, then 130 (data set 1), then 130 (data set 2), then 300."""
    calls = []
    for stop, key in enumerate((BIG, SMALL, "a130", "b130", BIG)):
        for e in SELECT:
            v = VARIANTS[e][(stop // 2) % len(VARIANTS[e])] if stop != 4 else VARIANTS[e][-1]
            calls.append(Call(e, v, key, form_of(e, key), SPEC if stop % 2 else None, None))
    return calls


def violations(calls):
    """The conditions a seeded schedule meets, as a list of what is missing (empty: all hold)."""
    bad = []
    ok = [c for c in calls if c.fail is None]
    # 1. every entry of the vocabulary occurs
    for e in ENTRIES:
        for v in VARIANTS[e]:
            if not any(c.entry == e and c.variant == v for c in ok):
                bad.append(f"{e}/{v} never runs")
    for e in SELECT:
        for kind in "ab":
            if not any(c.entry == e and c.fail == kind for c in calls):
                bad.append(f"{e} never fails with ({kind})")
    if not any(c.entry == "anosim" and c.fail == "c" for c in calls):
        bad.append("anosim never fails with (c)")
    for c in calls:
        if c.form != form_of(c.entry, c.data) or (c.fail in ("b", "c") and c.plan != SPEC) or \
                ((c.data == DUP) != (c.fail == "b")):
            bad.append(f"malformed call {c}")
    if not ({c.form for c in ok} >= {"f64", "f32", "csc"} and {c.plan for c in ok} == {None, SPEC}):
        bad.append("a form or a plan is never used")
    # 2. no successful call repeats its entry's previous successful call
    last = {}
    for i, c in enumerate(calls):
        if c.fail is None:
            if last.get(c.entry) == answer_key(c):
                bad.append(f"call {i} ({c.entry}) would find its own answer")
            last[c.entry] = answer_key(c)
    # 3. every selection entry directly after a larger, a smaller and the twin data set
    # 4. every entry directly after every other entry it shares a buffer with
    # 5. every kind of refused call directly before every follower
    seen_size, seen_after, seen_fail = set(), set(), set()
    for p, c in zip(calls, calls[1:]):
        if c.fail is not None:
            continue
        if p.fail is not None:
            seen_fail.add((p.fail, c.entry))
            continue
        seen_after.add((p.entry, c.entry))
        if p.entry != "pair":
            sp, sc = n_samp(p.data), n_samp(c.data)
            if sp > sc:
                seen_size.add((c.entry, "larger"))
            if sp < sc:
                seen_size.add((c.entry, "smaller"))
            if TWIN.get(c.data) == p.data:
                seen_size.add((c.entry, "twin"))
    for e in SELECT:
        for cond in ("larger", "smaller", "twin"):
            if (e, cond) not in seen_size:
                bad.append(f"{e} never directly follows {cond} data")
    for users in BUFFER_USERS.values():
        for e in users:
            for f in users:
                if e != f and (f, e) not in seen_after:
                    bad.append(f"{e} never directly follows {f}")
    for kind in FAIL_KINDS:
        for f in FOLLOWERS:
            if (kind, f) not in seen_fail:
                bad.append(f"{f} never directly follows a refused call of kind ({kind})")
    # 6. big, small, big
    sizes = [n_samp(c.data) for c in ok if c.entry != "pair"]
    small = [i for i, s in enumerate(sizes) if s == n_samp(SMALL)]
    big = [i for i, s in enumerate(sizes) if s == n_samp(BIG)]
    if not (small and big and any(big[0] < s < big[-1] for s in small)):
        bad.append("the largest shape does not occur before and after the smallest")
    return sorted(set(bad))


def hand_written_violations(calls):
    """What the hand-written schedule promises: the five stops in order, all eight selection entries at each, and no
    call that would find its own answer."""
    bad = []
    stops = [c.data for c in calls[::len(SELECT)]]
    if stops != [BIG, SMALL, "a130", "b130", BIG] or len(calls) != 5 * len(SELECT):
        bad.append(f"stops {stops}")
    for s in range(5):
        part = calls[s * len(SELECT):(s + 1) * len(SELECT)]
        if tuple(c.entry for c in part) != SELECT or {c.data for c in part} != {stops[s]} or any(c.fail for c in part):
            bad.append(f"stop {s}")
    last = {}
    for i, c in enumerate(calls):
        if last.get(c.entry) == answer_key(c):
            bad.append(f"call {i} ({c.entry}) would find its own answer")
        last[c.entry] = answer_key(c)
    return bad


def all_schedules():
    """name -> list of calls: the hand-written schedule and one per seed"""
    out = {"hand": hand_written()}
    for s in SEEDS:
        out[f"seed{s}"] = schedule(s)
    return out
