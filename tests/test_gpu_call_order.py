"""Every entry on a context that other calls have already used (tests/call_schedule.py: the inputs, the vocabulary and
the schedules; tests/test_call_schedule_host.py: what the schedules guarantee).

A context keeps its device buffers from call to call, so an entry is right only if it resets or rewrites everything it
reads (DESIGN.md section 16 lists it buffer by buffer).  Each schedule runs on ONE context of its own, in order, with
refused calls in between, and every successful result is compared bit for bit -- dtype, shape and bytes -- with the
same call on a fresh context, which has nothing before the call.  The fresh-context answers themselves are held to the
entries' brute-force checkers and to the CPU oracle, since the inputs are new to the suite."""
import numpy as np
import pytest

from icikendalltau_amd import _lib
from tests import call_schedule as cs
from tests import test_gpu_anosim, test_gpu_classmat, test_gpu_medians, test_gpu_mst, test_gpu_padjust
from tests import test_gpu_quantiles, test_gpu_topk
from tests.anosim_checker import brute_anosim
from tests.classmat_checker import brute_class_matrix
from tests.edges_checker import assert_same as edges_assert_same, brute_edges
from tests.medians_checker import brute_medians, class_pairs
from tests.mst_checker import brute_mst
from tests.padjust_checker import brute_padjust
from tests.quantiles_checker import brute_quantiles
from tests.test_gpu_select_shared import _same
from tests.topk_checker import brute_topk, ranked_partners

pytestmark = pytest.mark.gpu

ATOL = 1e-10          # BASELINE.json north_star: the four doubles against the CPU oracle
SCHEDULES = cs.all_schedules()


class Refs:
    """The answer of every distinct successful call of the schedules, each from a context created for it and closed
    behind it; for the entries of cs.DETERMINISM a second answer from a second fresh context."""

    def __init__(self):
        self.ref, self.second, self.values = {}, {}, {}
        for calls in SCHEDULES.values():
            for call in calls:
                if call.fail is None:
                    self.get(call)
        for key in cs.DATA:
            self.matrix(key)
        for k in list(self.ref):
            if k[0] in cs.DETERMINISM:
                self.second[k] = self._fresh(cs.Call(*k, None, None))
        self.disagree = [k for k, v in self.second.items() if not _same(v, self.ref[k])]

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

    def matrix(self, key):
        """(out5, max_taumax, reason_counts) of the data set's fresh matrix call"""
        out5, _keep, rc5 = self.get(cs.Call("matrix", "full", key, cs.form_of("matrix", key), None, None))
        tm = out5[3][np.triu_indices(out5.shape[1], k=1)]
        tm = tm[~np.isnan(tm)]
        return out5, (float(tm.max()) if tm.size else -np.inf), rc5

    def class_pairs_matrix(self, key):
        """(out5, max_taumax, reason_counts) of a fresh matrix call over the within-class pairs of cs.classes3, as
        tests/test_gpu_medians._reference computes it; without such a pair (S = 3) nothing is computed at all"""
        S = cs.n_samp(key)
        pi, pj = class_pairs(*cs.classes3(S))
        if len(pi) == 0:
            return np.full((5, S, S), np.nan), -np.inf, np.zeros(5, dtype=np.int64)
        ctx = _lib.Context(0)
        try:
            out5, _keep, rc5 = ctx.matrix(cs.matrix_in(key, cs.form_of("matrix", key)), None, pi, pj, want_keep=False)
        finally:
            ctx.close()
        tm = out5[3][pi, pj]
        tm = tm[~np.isnan(tm)]
        return out5, (float(tm.max()) if tm.size else -np.inf), rc5

    def resolve(self, name, key, _form):
        if key not in self.values:
            out5 = self.matrix(key)[0]
            raw = out5[1][np.triu_indices(out5.shape[1], k=1)]
            raw = raw[~np.isnan(raw)]
            self.values[key] = {"n_edges": int(np.sum(raw >= 0.0)), "median_raw": float(np.median(raw))}
        return self.values[key][name]


@pytest.fixture(scope="module")
def refs():
    return Refs()


def test_two_fresh_contexts_agree(refs):
    """the precondition of comparing cor_pairs and the three diagnostics bit for bit: they are pure functions of their
    input too (the other entries are documented as such)"""
    print("distinct fresh-context references", len(refs.ref), "of them computed twice", len(refs.second),
          "disagreeing", refs.disagree)
    assert {k[0] for k in refs.second} == set(cs.DETERMINISM)
    assert refs.disagree == []


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_schedule(refs, name):
    calls = SCHEDULES[name]
    ctx = _lib.Context(0)
    try:
        for i, call in enumerate(calls):
            ctx.debug_set_plan(call.plan)
            if call.fail:
                with pytest.raises(_lib.IciktError, match=cs.FAIL_MESSAGE[call.fail].format(who=call.entry)):
                    cs.run(ctx, call, refs.resolve)
                continue
            got = cs.run(ctx, call, refs.resolve)
            assert _same(got, refs.get(call)), (name, i, call, calls[max(i - 1, 0)])
        ctx.debug_set_plan(None)
        last = cs.Call("matrix", "full", "b130", cs.form_of("matrix", "b130"), None, None)
        assert _same(cs.run(ctx, last), refs.get(last)), (name, "the matrix call behind the schedule")
    finally:
        ctx.close()


def _sample(n, m=2000):
    return np.sort(np.random.default_rng(n).permutation(n)[:m])


def test_matrix_and_pairs_references_match_the_oracle(refs):
    """counts and reason codes exactly, the doubles within 1e-10, on up to 2 000 pairs per reference"""
    from oracle import oracle as O
    checked = 0
    for (entry, variant, key, _form), got in refs.ref.items():
        if entry not in ("matrix", "pairs"):
            continue
        X, S = cs.dense(key), cs.n_samp(key)
        iu, ju = np.triu_indices(S, k=1)
        if entry == "pairs" and variant == "list":
            iu, ju = cs.pair_list(S)
        ref, rcnt, rrsn = O.ici_pairs(X, iu, ju, "global")
        sel = _sample(len(iu))
        if entry == "matrix":
            out5, _keep, rc5 = got
            assert np.array_equal(rc5, np.bincount(rrsn, minlength=5))
            out = np.stack([out5[q][iu[sel], ju[sel]] for q in (1, 2, 3, 4)], axis=1)
            assert np.array_equal(np.isnan(out[:, 0]), rrsn[sel] != 0)
        else:
            out, cnt, rsn = got
            assert np.array_equal(rsn, rrsn)
            ok = rrsn[sel] == 0
            assert np.array_equal(cnt[sel][ok], rcnt[sel][ok][:, :cnt.shape[1]])
            out = out[sel]
        assert np.array_equal(np.isnan(out), np.isnan(ref[sel]))
        same = out == ref[sel]                      # (an infinite value on both sides has no difference)
        with np.errstate(invalid="ignore"):         # (NA_real_ is a signalling NaN)
            d = float(np.nanmax(np.abs(np.where(same, 0.0, out) - np.where(same, 0.0, ref[sel])), initial=0.0))
        print(entry, variant, key, "pairs", len(sel), "largest difference", d)
        assert d <= ATOL
        checked += 1
    assert checked >= len(cs.DATA) + 2


def test_selection_references_pass_their_checkers(refs):
    """each fresh reference of a selection entry through that entry's brute-force checker on the fresh matrix of the
    same data, with the entry suite's own comparison (bitwise doubles, exact integers)"""
    seen = set()
    ranked = {}
    for (entry, variant, key, form), got in refs.ref.items():
        if entry not in cs.SELECT:
            continue
        out5, mx, rc5 = refs.matrix(key)
        S = cs.n_samp(key)
        seen.add((entry, variant))
        if entry == "topk":
            if key not in ranked:
                ranked[key] = ranked_partners(out5[1])
            test_gpu_topk._assert_same(got, brute_topk(out5, 1 if variant == "k1" else 7, ranked[key]))
            assert got[3] == mx and np.array_equal(got[4], rc5)
        elif entry == "edges":
            ref = brute_edges(out5, min_raw=0.0)
            m = refs.resolve("n_edges", key, form)
            assert m == ref[3] >= 1                 # max_edges equal to the number of edges ...
            if variant == "short":
                m = max(m // 3, 1)                  # ... and smaller (S = 3 has one edge: no smaller list)
                assert m < ref[3] or S == 3
            edges_assert_same(got, ref, max_edges=m)
            assert len(got[0]) == m and got[5] == mx and np.array_equal(got[6], rc5)
        elif entry == "class_medians" and variant == "one":
            test_gpu_medians._assert_same(got, brute_medians(out5, None) + (mx, rc5))
        elif entry == "class_medians":
            # only the within-class pairs are computed: cor's denominator and the reason counts are theirs
            cls, n_class = cs.classes3(S)
            o5, cmx, crc = refs.class_pairs_matrix(key)
            test_gpu_medians._assert_same(got, brute_medians(o5, cls) + (cmx, crc))
        elif entry == "class_matrix":
            test_gpu_classmat._assert_same(got, brute_class_matrix(out5, *cs.classes3(S)) + (mx, rc5))
        elif entry == "quantiles":
            args = ((None, (), cs.BREAKS) if variant == "hist" else (cs.classes3(S)[0], cs.PROBS, cs.BREAKS))
            test_gpu_quantiles._assert_same(got, brute_quantiles(out5, *args) + (mx, rc5))
        elif entry == "padjust":
            ref = brute_padjust(out5[2], variant, cs.ALPHAS)
            ref["max_taumax"], ref["reason_counts"] = mx, rc5
            test_gpu_padjust._assert_same(got, ref)
        elif entry == "mst":
            thr = None if variant == "all" else refs.resolve("median_raw", key, form)
            test_gpu_mst._assert_same(got, ((out5, mx, rc5), brute_mst(out5[1], thr)))
        else:
            cls, n_class, perms = cs.labellings(S)
            test_gpu_anosim._assert_same(got, ((out5[1], mx, rc5), brute_anosim(out5[1], cls, n_class, perms)))
    assert seen == {(e, v) for e in cs.SELECT for v in cs.VARIANTS[e]}
