"""The library on a caller's stream (icikt_ctx_set_stream): the device-resident calls in stream order with no host
synchronisation between them, and every host entry on a stream that is still busy (tests/stream_cases.py: the cases;
tests/test_stream_cases_host.py: what the oracle says about them).

include/icikt.h, "Stream contract": a device-resident call is work on the context's stream at the place of the call.
The test puts the library between torch work on the SAME stream and lets nothing but the stream order them:

    gate | dX <- true | prepare_dev | run_dev global | run_dev local | dX <- decoy | snapshots | outputs <- sentinel

The gate is a chain of float64 matmuls whose length is measured (the `gate` fixture) and chosen, per case, as at least
50 times the host time the same calls took to enqueue before -- so everything behind it is enqueued while dX still holds
the decoy and the library's buffers still hold the prepared DECOY matrix, its pair counts and its results (a step on the
decoy runs before the gated step: stale state is never the right answer).  A library that reads dX or one of its own
buffers before its place in the stream computes from the decoy, whose tau differs in every pair; one that writes after
its place misses the snapshot or overwrites the sentinel.  The snapshots are compared bit for bit with a synchronous
step on the same context, which is held to the CPU oracle (counts and reasons exactly, the doubles within 1e-10).

`pending`: whether the gate was still running when the last call had returned -- true where the contract says the calls
return before the stream reaches them, false where it names a synchronisation.  Asserted as the header states it."""
import math
import time
from collections import namedtuple

import numpy as np
import pytest

from icikendalltau_amd import _lib
from tests import call_schedule as cs
from tests import stream_cases as sc
from tests.test_gpu_select_shared import _same

pytestmark = pytest.mark.gpu

ATOL = 1e-10              # BASELINE.json north_star: the four doubles against the CPU oracle
GATE_FACTOR = 50          # the gate lasts at least this many times the host's enqueue time of the calls behind it ...
GATE_CAP_S = 0.5          # ... and at most this long
HOST_GATE_S = 0.01        # the gate in front of a host entry
KINDS = ("own", "null", "null-none", "side", "side-high")
S, P = sc.S, sc.PAIRS
TRUE, DECOY = "true", "decoy"


def run_dev_synchronises(n):
    """include/icikt.h, "Stream contract": the first icikt_run_dev behind a pre-pass reads the column statistics back
    for columns of 14 273 to 65 535 rows (csrc/icikt_pipeline.cpp: matrix_tied; k1_half_items(Wp) >= 9, not wide)."""
    return 14272 < n <= 65535


# ---- the gate --------------------------------------------------------------------------------------------------------

class Gate:
    """`units` float64 matmuls of N x N on the current stream: ordinary work whose length is fixed by its size.  The
    time of one unit is measured once, with torch events."""
    N = 2048

    def __init__(self):
        import torch
        self.a = torch.rand((self.N, self.N), dtype=torch.float64, device="cuda")
        self.b = torch.rand((self.N, self.N), dtype=torch.float64, device="cuda")
        self.c = torch.empty((self.N, self.N), dtype=torch.float64, device="cuda")
        self.run(3)
        torch.cuda.synchronize()
        reps = 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        self.run(reps)
        self.unit_enqueue_s = (time.perf_counter() - t0) / reps
        e1.record()
        e1.synchronize()
        self.unit_s = e0.elapsed_time(e1) * 1e-3 / reps
        print(f"\ngate: one {self.N} x {self.N} float64 matmul lasts {self.unit_s * 1e6:.0f} us on the device and takes "
              f"{self.unit_enqueue_s * 1e6:.0f} us to enqueue")

    def run(self, units):
        import torch
        for _ in range(units):
            torch.mm(self.a, self.b, out=self.c)

    def sized(self, enqueue_s):
        """(units, seconds) of the gate for calls that took enqueue_s to enqueue"""
        want = min(GATE_FACTOR * enqueue_s, GATE_CAP_S)
        units = max(1, math.ceil(want / self.unit_s))
        if units * self.unit_s > GATE_CAP_S:
            units = max(1, int(GATE_CAP_S / self.unit_s))
        return units, units * self.unit_s

    def seconds(self, s):
        return max(1, math.ceil(s / self.unit_s))


@pytest.fixture(scope="module")
def gate():
    g = Gate()
    # a unit must outlast its own enqueue by far, or the host could not queue work behind a running gate
    assert g.unit_s > 4 * g.unit_enqueue_s, (g.unit_s, g.unit_enqueue_s)
    return g


# ---- a context on a stream of one kind ----------------------------------------------------------------------------------

class Lane:
    """A context and the torch stream its caller works on.  own: the context keeps its own non-blocking stream, the
    caller works on torch's default stream, and a host synchronisation stands wherever work passes from one to the
    other (the baseline: what every other GPU test of the device-resident path does).  Every other kind: the context is
    put on the caller's stream and nothing but that stream orders the two."""

    def __init__(self, ctx, kind, ts=None):
        import torch
        self.ctx, self.kind, self.ordered = ctx, kind, kind != "own"
        if kind in ("side", "side-high"):
            self.ts = ts or (torch.cuda.Stream(priority=-1) if kind == "side-high" else torch.cuda.Stream())
            assert self.ts.cuda_stream != 0
            ctx.set_stream(self.ts.cuda_stream)
        else:
            self.ts = torch.cuda.default_stream()
            if kind == "null":
                handle = torch.cuda.current_stream().cuda_stream          # as bench.py passes it
                assert handle == 0
                ctx.set_stream(handle)
            elif kind == "null-none":
                ctx.set_stream(None)
            else:
                ctx.use_own_stream()

    def to_lib(self):
        if not self.ordered:
            self.ts.synchronize()

    def to_torch(self):
        if not self.ordered:
            self.ctx.sync()

    def warm(self, gate):
        """the first matmul on a stream sets up the BLAS library's state for it"""
        import torch
        with torch.cuda.stream(self.ts):
            gate.run(1)
        self.ts.synchronize()


class Bufs:
    """The device tensors of one case: the true and the decoy matrix ([S, n] row-major = n x S column-major), dX, the
    six outputs of a step (out4, counts, reasons of the global and of the local run) and their snapshots.  f32: a
    float32 row-major source [n, S] beside them, for icikt_convert_dev."""

    def __init__(self, X_true, X_decoy, f32=False):
        import torch
        self.n = X_true.shape[0]
        self.d = {k: torch.from_numpy(np.array(M.T, order="C")).cuda() for k, M in ((TRUE, X_true), (DECOY, X_decoy))}
        self.dX = torch.empty_like(self.d[TRUE])
        self.d32 = self.src32 = None
        if f32:
            self.d32 = {k: torch.from_numpy(np.ascontiguousarray(M, dtype=np.float32)).cuda()
                        for k, M in ((TRUE, X_true), (DECOY, X_decoy))}
            self.src32 = torch.empty_like(self.d32[TRUE])
        self.out = []
        for _persp in range(2):
            self.out += [torch.empty((P, 4), dtype=torch.float64, device="cuda"),
                         torch.empty((P, len(_lib.CNT_FIELDS)), dtype=torch.int64, device="cuda"),
                         torch.empty(P, dtype=torch.int32, device="cuda")]
        self.snap = [torch.empty_like(o) for o in self.out]
        self.fill()
        torch.cuda.synchronize()

    def load(self, which):
        self.dX.copy_(self.d[which])
        if self.src32 is not None:
            self.src32.copy_(self.d32[which])

    def fill(self):
        for o in self.out:
            o.fill_(sc.SENTINEL)

    def take(self):
        for s, o in zip(self.snap, self.out):
            s.copy_(o)

    def ptr(self, i):
        return self.out[i].data_ptr()


def feed_plain(lane, B, flags):
    lane.ctx.prepare_dev(B.dX.data_ptr(), B.n, S, B.n, flags)


def feed_convert(lane, B, flags):
    """a float32 row-major source through icikt_convert_dev (dX is written by the library, not by the caller)"""
    lane.ctx.convert_dev(B.src32.data_ptr(), _lib.DTYPE_F32, _lib.ORDER_ROW, B.n, S, S, B.dX.data_ptr(), B.n)
    lane.ctx.prepare_dev(B.dX.data_ptr(), B.n, S, B.n, flags)


def feed_ranks(lane, B, flags):
    """the sharded pre-pass of three ranks, one context playing them in turn, then the rebuild of all columns"""
    ranges, alloc = sc.rank_ranges(3)
    for c0, c1 in ranges:
        lane.ctx.prepare_cols_dev(B.dX.data_ptr(), B.n, S, B.n, c0, c1, alloc, flags)
    lane.ctx.expand_cols_dev(0, S, flags)


Step = namedtuple("Step", "got left pending enqueue_s")


def run_step(lane, B, which, gate=None, units=0, flags=0, feed=feed_plain):
    """One step on `lane` (module docstring).  got: the six snapshots; left: the six output tensors after the step;
    pending: whether the gate was still running when everything had been enqueued (None without a gate); enqueue_s:
    the host time from the first call behind the gate to the last."""
    import torch
    ctx = lane.ctx
    with torch.cuda.stream(lane.ts):
        e_gate = None
        if units:
            gate.run(units)
            e_gate = torch.cuda.Event()
            e_gate.record()
        t0 = time.perf_counter()
        B.load(which)
        lane.to_lib()
        feed(lane, B, flags)
        ctx.run_dev(1, 0, False, flags, B.ptr(0), B.ptr(1), B.ptr(2))
        ctx.run_dev(0, 0, False, flags | _lib.FLAG_REUSE_COUNTS, B.ptr(3), B.ptr(4), B.ptr(5))
        lane.to_torch()
        B.load(DECOY)                       # the header: dX is the caller's again from here on
        B.take()
        B.fill()
        enqueue_s = time.perf_counter() - t0
        pending = None if e_gate is None else not e_gate.query()
        lane.ts.synchronize()
    torch.cuda.synchronize()
    return Step(tuple(s.cpu().numpy() for s in B.snap), tuple(o.cpu().numpy() for o in B.out), pending, enqueue_s)


def assert_untouched(left, label):
    for i, a in enumerate(left):
        assert np.all(a == a.dtype.type(sc.SENTINEL)), (label, "output", i, "was written behind the library's place")


def assert_oracle(got, ref, label):
    """counts and reasons exactly, the doubles within ATOL"""
    for k, persp in enumerate(("global", "local")):
        out, cnt, rsn = got[3 * k:3 * k + 3]
        rout, rcnt, rrsn = ref[persp]
        assert np.array_equal(rsn, rrsn), (label, persp)
        assert np.array_equal(cnt, rcnt[:, :cnt.shape[1]]), (label, persp)
        d = float(np.max(np.abs(out - rout)))
        assert d <= ATOL, (label, persp, d)


def warm_up(lane, B, gate, ref, ref_decoy, label, feed=feed_plain):
    """The synchronous steps in front of a gated one: a step on the true matrix, which makes the allocations and uploads
    the task list and is itself held to the oracle, and a step on the decoy, which leaves the decoy's prepared state,
    counts and results in the library's buffers.  Returns (the true step, the host's enqueue time: the longer of the
    two steps')."""
    lane.warm(gate)
    warm = run_step(lane, B, TRUE, feed=feed)
    assert_oracle(warm.got, ref, label + ("warm",))
    assert_untouched(warm.left, label + ("warm",))
    dec = run_step(lane, B, DECOY, feed=feed)
    assert_oracle(dec.got, ref_decoy, label + ("decoy",))
    assert not any(_same(a, b) for a, b in zip(warm.got[::3], dec.got[::3]))
    return warm, max(warm.enqueue_s, dec.enqueue_s)


def gated_step(lane, B, gate, warm, enqueue_s, label, feed=feed_plain, expect_pending=None):
    units, gate_s = gate.sized(enqueue_s)
    res = run_step(lane, B, TRUE, gate, units, feed=feed)
    print(f"\n{label}: enqueue before {enqueue_s * 1e6:.0f} us, gate {units} units = {gate_s * 1e3:.1f} ms, "
          f"enqueue behind the gate {res.enqueue_s * 1e6:.0f} us, pending {res.pending}")
    assert _same(res.got, warm.got), (label, "a snapshot differs from the synchronous step")
    assert_untouched(res.left, label)
    if expect_pending is not None:
        assert res.pending is expect_pending, (label, "pending", res.pending, "the header says", expect_pending)
    return res


# ---- (a) the ordered step behind a gate -----------------------------------------------------------------------------------

A_CASES = [(case, kind) for case in sc.CASES for kind in (KINDS if case.n in sc.ALL_KINDS_AT else ("side",))]


@pytest.mark.parametrize("case,kind", A_CASES, ids=[f"{sc.case_id(c)}-{k}" for c, k in A_CASES])
def test_ordered_step(gate, case, kind):
    ctx = _lib.Context(0)
    try:
        B = Bufs(sc.true_matrix(case), sc.decoy_matrix(case))
        lane = Lane(ctx, kind)
        ctx.set_pairs_combn(S, 0, P)
        label = (sc.case_id(case), kind)
        warm, enq = warm_up(lane, B, gate, sc.reference(case), sc.decoy_reference(case), label)
        if not lane.ordered:
            # the baseline has no stream order to test: a third synchronous step, from the decoy's state
            res = run_step(lane, B, TRUE)
            assert _same(res.got, warm.got), label
            assert_untouched(res.left, label)
            return
        gated_step(lane, B, gate, warm, enq, label, expect_pending=not run_dev_synchronises(case.n))
        if kind in ("side", "side-high"):
            # Once more on a second stream of the same kind.  The runtime maps streams onto a few hardware queues, and
            # two streams that share one run in order whatever the library asked for: work the library put on a
            # stream of its own by mistake is invisible while that stream shares the caller's queue (measured: with the
            # epilogue moved to the context's own stream 8 of the 18 side-stream cases passed on one stream, none on
            # two).  Streams created one after the other are spread over the queues.
            lane = Lane(ctx, kind)
            lane.warm(gate)
            run_step(lane, B, DECOY)
            gated_step(lane, B, gate, warm, enq, label + ("second stream",),
                       expect_pending=not run_dev_synchronises(case.n))
    finally:
        ctx.close()


# ---- (b) the other device-resident calls ----------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_convert_dev_feeds_prepare_dev(gate, variant):
    case = sc.Case(700, variant)
    X, D = sc.as_float32(sc.true_matrix(case)), sc.as_float32(sc.decoy_matrix(case))
    ctx = _lib.Context(0)
    try:
        B = Bufs(X, D, f32=True)
        lane = Lane(ctx, "side")
        ctx.set_pairs_combn(S, 0, P)
        label = (sc.case_id(case), "convert_dev")
        warm, enq = warm_up(lane, B, gate, sc.oracle_answers(X), sc.oracle_answers(D), label, feed=feed_convert)
        gated_step(lane, B, gate, warm, enq, label, feed=feed_convert, expect_pending=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [700, 10000])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_rank_ranges_then_expand(gate, variant, n):
    case = sc.Case(n, variant)
    ctx = _lib.Context(0)
    try:
        B = Bufs(sc.true_matrix(case), sc.decoy_matrix(case))
        lane = Lane(ctx, "side")
        ctx.set_pairs_combn(S, 0, P)
        label = (sc.case_id(case), "prepare_cols_dev x 3, expand_cols_dev")
        warm, enq = warm_up(lane, B, gate, sc.reference(case), sc.decoy_reference(case), label, feed=feed_ranks)
        gated_step(lane, B, gate, warm, enq, label, feed=feed_ranks, expect_pending=True)
        # ... and the sharded pre-pass leaves what the whole one leaves
        plain = run_step(lane, B, TRUE)
        assert _same(plain.got, warm.got), label
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [700, 20000])
def test_combn_blocks_without_a_sync_between(gate, n):
    """The sharding unit of test_combn_ranges_concatenate_to_full without its sync() per block: three consecutive
    blocks of the pair list, a run after each into its own buffer.  Every run follows a new pair list, so every one
    uploads a task list and synchronises (the header says so): the gate is over when the calls have returned."""
    import torch
    case = sc.Case(n, "continuous")
    ctx = _lib.Context(0)
    try:
        B = Bufs(sc.true_matrix(case), sc.decoy_matrix(case))
        lane = Lane(ctx, "side")
        ctx.set_pairs_combn(S, 0, P)
        label = (sc.case_id(case), "combn blocks")
        warm, enq = warm_up(lane, B, gate, sc.reference(case), sc.decoy_reference(case), label)
        blocks = sc.combn_blocks(3)
        outs = [torch.full((e - b, 4), sc.SENTINEL, dtype=torch.float64, device="cuda") for b, e in blocks]
        snaps = [torch.empty_like(o) for o in outs]
        torch.cuda.synchronize()

        def sequence(which, units):
            with torch.cuda.stream(lane.ts):
                e_gate = None
                if units:
                    gate.run(units)
                    e_gate = torch.cuda.Event()
                    e_gate.record()
                B.load(which)
                ctx.prepare_dev(B.dX.data_ptr(), n, S, n)
                for (b, e), o in zip(blocks, outs):
                    ctx.set_pairs_combn(S, b, e)
                    ctx.run_dev(1, 0, False, 0, o.data_ptr())
                B.load(DECOY)
                for s, o in zip(snaps, outs):
                    s.copy_(o)
                    o.fill_(sc.SENTINEL)
                pending = None if e_gate is None else not e_gate.query()
                lane.ts.synchronize()
            torch.cuda.synchronize()
            return np.concatenate([s.cpu().numpy() for s in snaps]), pending

        first, _ = sequence(TRUE, 0)
        assert _same(first, warm.got[0]), label
        dec, _ = sequence(DECOY, 0)
        assert not _same(dec, first)
        got, pending = sequence(TRUE, gate.sized(enq)[0])
        assert _same(got, warm.got[0]), label
        assert all(bool(torch.all(o == sc.SENTINEL)) for o in outs), label
        print(f"\n{label}: pending {pending}")
        assert pending is False, label
    finally:
        ctx.close()


def test_set_pairs_behind_a_gated_run(gate):
    """icikt_set_pairs with a shuffled explicit list directly behind a run of the combn list that the gate still
    holds back: the re-upload of d_pi / d_pj (and, in the next run, of the task list) must not reach the first run."""
    import torch
    case = sc.Case(700, "tied")
    perm, pi, pj = sc.shuffled_pairs()
    ctx = _lib.Context(0)
    try:
        B = Bufs(sc.true_matrix(case), sc.decoy_matrix(case))
        lane = Lane(ctx, "side")
        ctx.set_pairs_combn(S, 0, P)
        label = (sc.case_id(case), "set_pairs behind a run")
        warm, enq = warm_up(lane, B, gate, sc.reference(case), sc.decoy_reference(case), label)
        out_b = torch.full((P, 4), sc.SENTINEL, dtype=torch.float64, device="cuda")
        snap_b = torch.empty_like(out_b)
        torch.cuda.synchronize()

        def sequence(units):
            # the combn list again, its task list uploaded, and the decoy's state in the library's buffers
            ctx.set_pairs_combn(S, 0, P)
            run_step(lane, B, DECOY)
            with torch.cuda.stream(lane.ts):
                e_gate = None
                if units:
                    gate.run(units)
                    e_gate = torch.cuda.Event()
                    e_gate.record()
                B.load(TRUE)
                ctx.prepare_dev(B.dX.data_ptr(), B.n, S, B.n)
                ctx.run_dev(1, 0, False, 0, B.ptr(0), B.ptr(1), B.ptr(2))
                held = None if e_gate is None else not e_gate.query()
                ctx.set_pairs(pi, pj)
                ctx.run_dev(1, 0, False, 0, out_b.data_ptr())
                B.load(DECOY)
                B.take()
                snap_b.copy_(out_b)
                B.fill()
                out_b.fill_(sc.SENTINEL)
                lane.ts.synchronize()
            torch.cuda.synchronize()
            return tuple(s.cpu().numpy() for s in B.snap[:3]), snap_b.cpu().numpy(), held

        sequence(0)
        first, second, held = sequence(gate.sized(enq)[0])
        assert held is True, (label, "the first run was not held back by the gate when set_pairs was called")
        assert _same(first, warm.got[:3]), (label, "the first run saw the second list")
        assert _same(second, np.ascontiguousarray(warm.got[0][perm])), label
        assert bool(torch.all(out_b == sc.SENTINEL)), label
    finally:
        ctx.close()


# ---- (c) switching streams --------------------------------------------------------------------------------------------------

def test_prepare_on_one_stream_run_on_another_then_null_then_own(gate):
    """icikt_ctx_set_stream / icikt_ctx_use_own_stream drain the stream the context leaves (the header says so): the
    pre-pass enqueued on stream A is complete when the first call on stream B is made."""
    import torch
    case = sc.Case(700, "continuous")
    ctx = _lib.Context(0)
    try:
        B = Bufs(sc.true_matrix(case), sc.decoy_matrix(case))
        lane_a = Lane(ctx, "side")
        ctx.set_pairs_combn(S, 0, P)
        label = (sc.case_id(case), "A -> B -> null -> own")
        warm, enq = warm_up(lane_a, B, gate, sc.reference(case), sc.decoy_reference(case), label)
        stream_b = torch.cuda.Stream()
        with torch.cuda.stream(stream_b):
            gate.run(1)
        stream_b.synchronize()
        with torch.cuda.stream(lane_a.ts):
            gate.run(gate.sized(enq)[0])
            e_gate = torch.cuda.Event()
            e_gate.record()
            B.load(TRUE)
            ctx.prepare_dev(B.dX.data_ptr(), B.n, S, B.n)
            held = not e_gate.query()
        ctx.set_stream(stream_b.cuda_stream)
        assert held and e_gate.query(), (label, "set_stream left work behind on the stream it switched from")
        with torch.cuda.stream(stream_b):
            ctx.run_dev(1, 0, False, 0, B.ptr(0), B.ptr(1), B.ptr(2))
            ctx.run_dev(0, 0, False, _lib.FLAG_REUSE_COUNTS, B.ptr(3), B.ptr(4), B.ptr(5))
            B.load(DECOY)
            B.take()
            B.fill()
            stream_b.synchronize()
        torch.cuda.synchronize()
        assert _same(tuple(s.cpu().numpy() for s in B.snap), warm.got), (label, "run on B")
        assert_untouched(tuple(o.cpu().numpy() for o in B.out), label)
        for kind in ("null-none", "own"):
            lane = Lane(ctx, kind)
            run_step(lane, B, DECOY)
            if lane.ordered:
                gated_step(lane, B, gate, warm, enq, label + (kind,), expect_pending=True)
            else:
                res = run_step(lane, B, TRUE)
                assert _same(res.got, warm.got), label + (kind,)
                assert_untouched(res.left, label + (kind,))
    finally:
        ctx.close()


def test_two_contexts_on_one_stream(gate):
    import torch
    cases = (sc.Case(700, "continuous"), sc.Case(10000, "tied"))
    ts = torch.cuda.Stream()
    ctxs = [_lib.Context(0), _lib.Context(0)]
    try:
        lanes, bufs, warms, enq = [], [], [], 0.0
        for ctx, case in zip(ctxs, cases):
            B = Bufs(sc.true_matrix(case), sc.decoy_matrix(case))
            lane = Lane(ctx, "side", ts)
            ctx.set_pairs_combn(S, 0, P)
            warm, e = warm_up(lane, B, gate, sc.reference(case), sc.decoy_reference(case), (sc.case_id(case), "two contexts"))
            lanes.append(lane), bufs.append(B), warms.append(warm)
            enq += e
        with torch.cuda.stream(ts):
            gate.run(gate.sized(enq)[0])
            e_gate = torch.cuda.Event()
            e_gate.record()
            for B in bufs:
                B.load(TRUE)
            for ctx, B in zip(ctxs, bufs):
                ctx.prepare_dev(B.dX.data_ptr(), B.n, S, B.n)
            for ctx, B in zip(ctxs, bufs):
                ctx.run_dev(1, 0, False, 0, B.ptr(0), B.ptr(1), B.ptr(2))
            for ctx, B in zip(ctxs, bufs):
                ctx.run_dev(0, 0, False, _lib.FLAG_REUSE_COUNTS, B.ptr(3), B.ptr(4), B.ptr(5))
            for B in bufs:
                B.load(DECOY)
                B.take()
                B.fill()
            pending = not e_gate.query()
            ts.synchronize()
        torch.cuda.synchronize()
        print(f"\ntwo contexts on one stream: pending {pending}")
        assert pending is True
        for B, warm, case in zip(bufs, warms, cases):
            assert _same(tuple(s.cpu().numpy() for s in B.snap), warm.got), sc.case_id(case)
            assert_untouched(tuple(o.cpu().numpy() for o in B.out), sc.case_id(case))
    finally:
        for ctx in ctxs:
            ctx.close()


def test_close_on_a_side_stream_with_work_in_flight(gate):
    """icikt_ctx_destroy drains the stream the context is on before it frees a buffer; the stream is the caller's and
    stays usable."""
    import torch
    case = sc.Case(700, "continuous")
    ctx = _lib.Context(0)
    try:
        B = Bufs(sc.true_matrix(case), sc.decoy_matrix(case))
        lane = Lane(ctx, "side")
        ctx.set_pairs_combn(S, 0, P)
        label = (sc.case_id(case), "close")
        warm, enq = warm_up(lane, B, gate, sc.reference(case), sc.decoy_reference(case), label)
        with torch.cuda.stream(lane.ts):
            gate.run(gate.sized(enq)[0])
            e_gate = torch.cuda.Event()
            e_gate.record()
            B.load(TRUE)
            ctx.prepare_dev(B.dX.data_ptr(), B.n, S, B.n)
            ctx.run_dev(1, 0, False, 0, B.ptr(0), B.ptr(1), B.ptr(2))
            ctx.run_dev(0, 0, False, _lib.FLAG_REUSE_COUNTS, B.ptr(3), B.ptr(4), B.ptr(5))
            held = not e_gate.query()
            ctx.close()
            assert held and e_gate.query(), label
            B.take()
            four = torch.ones(4, dtype=torch.float64, device="cuda").sum()
            lane.ts.synchronize()
        torch.cuda.synchronize()
        assert float(four) == 4.0
        assert _same(tuple(s.cpu().numpy() for s in B.snap), warm.got), label
    finally:
        ctx.close()


# ---- (d) the timers -----------------------------------------------------------------------------------------------------------

def _timed_step(kind, case, gate):
    """(launch counts, times in ms, the torch-event bracket in ms) of one step with ICIKT_FLAG_TIMING"""
    import torch
    ctx = _lib.Context(0)
    try:
        B = Bufs(sc.true_matrix(case), sc.decoy_matrix(case))
        lane = Lane(ctx, kind)
        ctx.set_pairs_combn(S, 0, P)
        label = (sc.case_id(case), kind, "timers")
        warm, _enq = warm_up(lane, B, gate, sc.reference(case), sc.decoy_reference(case), label)
        ctx.reset_timers()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(lane.ts):
            e0.record()
        res = run_step(lane, B, TRUE, flags=_lib.FLAG_TIMING)
        with torch.cuda.stream(lane.ts):
            e1.record()
        e1.synchronize()
        assert _same(res.got, warm.got), label
        figures = [ctx.kernel_ms(k) for k in (_lib.K_PREPARE, _lib.K_PAIRS, _lib.K_EPILOGUE)]
        return [f[1] for f in figures], [f[0] for f in figures], e0.elapsed_time(e1)
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [700, 10000])
@pytest.mark.parametrize("kind", ["side", "null"])
def test_timers_on_a_caller_stream(gate, kind, n):
    case = sc.Case(n, "tied")
    own_counts, own_ms, _ = _timed_step("own", case, gate)
    counts, ms, bracket = _timed_step(kind, case, gate)
    print(f"\ntimers {sc.case_id(case)} {kind}: launches {counts} (own stream {own_counts}), kernel_ms "
          f"{[round(v, 4) for v in ms]} (own stream {[round(v, 4) for v in own_ms]}), torch events around the step "
          f"{bracket:.4f} ms")
    assert own_counts == [1, 1, 2]                # one pre-pass, one pair-kernel launch, two epilogues
    assert counts == own_counts
    for v in ms + own_ms:
        assert np.isfinite(v) and v > 0.0


# ---- (e) every host entry on a caller's stream ----------------------------------------------------------------------------------

class FreshRefs:
    """The answer of a call on a context created for it, on its own stream, and closed behind it: the reference
    tests/test_gpu_call_order.py compares with, and holds to the entries' checkers and to the oracle for the same data
    and variants."""

    def __init__(self):
        self.ref, self.values = {}, {}

    def _fresh(self, call):
        if call.entry in ("edges", "mst"):
            self.resolve("n_edges", call.data, call.form)      # (from the data's matrix reference: before this context exists)
        ctx = _lib.Context(0)
        try:
            return cs.run(ctx, call, self.resolve)
        finally:
            ctx.close()

    def get(self, call):
        k = cs.ref_key(call)
        if k not in self.ref:
            self.ref[k] = self._fresh(call._replace(plan=None))
        return self.ref[k]

    def resolve(self, name, key, _form):
        if key not in self.values:
            out5 = self.get(cs.Call("matrix", "full", key, cs.form_of("matrix", key), None, None))[0]
            raw = out5[1][np.triu_indices(out5.shape[1], k=1)]
            raw = raw[~np.isnan(raw)]
            self.values[key] = {"n_edges": int(np.sum(raw >= 0.0)), "median_raw": float(np.median(raw))}
        return self.values[key][name]

    def hclust(self, method):
        k = ("hclust", method)
        if k not in self.ref:
            ctx = _lib.Context(0)
            try:
                self.ref[k] = ctx.hclust(cs.matrix_in("a130", "f64"), method)
            finally:
                ctx.close()
        return self.ref[k]


@pytest.fixture(scope="module")
def fresh():
    return FreshRefs()


def _gated(lane, gate, call_it, label):
    """call_it() with a gate running on the context's stream: the entry may not return before the stream has reached it"""
    import torch
    with torch.cuda.stream(lane.ts):
        gate.run(gate.seconds(HOST_GATE_S))
        e_gate = torch.cuda.Event()
        e_gate.record()
        held = not e_gate.query()
    got = call_it()
    assert held, (label, "the gate was over before the call")
    assert e_gate.query(), (label, "returned before the stream it was told to use had reached it")
    return got


def _host_schedule(name):
    if name == "hand":
        return cs.hand_written()
    return [cs.Call(e, v, key, cs.form_of(e, key), None, None)
            for e in cs.OTHER for v in cs.VARIANTS[e] for key in ("a130", "b65")]


@pytest.mark.parametrize("name", ["hand", "other"])
@pytest.mark.parametrize("kind", ["null", "side"])
def test_host_entries_on_a_caller_stream(gate, fresh, kind, name):
    calls = _host_schedule(name)
    assert len(calls) == (40 if name == "hand" else 2 * sum(len(cs.VARIANTS[e]) for e in cs.OTHER))
    refs = [fresh.get(call) for call in calls]
    ctx = _lib.Context(0)
    try:
        lane = Lane(ctx, kind)
        lane.warm(gate)
        gated = set()
        for i, (call, ref) in enumerate(zip(calls, refs)):
            ctx.debug_set_plan(call.plan)
            label = (kind, name, i, call)
            if call.entry in gated:
                got = cs.run(ctx, call, fresh.resolve)
            else:
                gated.add(call.entry)
                got = _gated(lane, gate, lambda: cs.run(ctx, call, fresh.resolve), label)
            assert _same(got, ref), label
        assert gated == set(cs.SELECT if name == "hand" else cs.OTHER)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["null", "side"])
def test_hclust_on_a_caller_stream(gate, fresh, kind):
    X = cs.matrix_in("a130", "f64")
    refs = {m: fresh.hclust(m) for m in _lib.HCLUST}
    ctx = _lib.Context(0)
    try:
        lane = Lane(ctx, kind)
        lane.warm(gate)
        for i, method in enumerate(("complete", "average", "single")):
            label = (kind, "hclust", method)
            got = _gated(lane, gate, lambda: ctx.hclust(X, method), label) if i == 0 else ctx.hclust(X, method)
            assert _same(got, refs[method]), label
    finally:
        ctx.close()
