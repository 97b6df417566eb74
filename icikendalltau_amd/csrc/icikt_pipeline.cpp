// icikt_pipeline.cpp -- what enqueues copies, the pre-pass (icikt_prepass.hip) and the pair kernels (icikt_kernels.hip)
// for the pair engine's entries (icikt_capi.cpp) and the drivers built on them (icikt_capi_select.cpp, icikt_multi.cpp):
// the prepared state's allocation and the pre-pass launches, the read-back behind the tie verdict (matrix_tied), the pair
// and task lists' way to the device, one launch of the pair kernel (launch_pair_tasks), the counts step of icikt_run_dev,
// and the host entries' transfer / pre-pass / pair pipeline (upload_and_prepare, upload_prepare_pairs).  The arithmetic
// behind all of it -- the launch plan, the task lists and their slices by chunk, a chunk's width, the pre-pass shape --
// is host-only code in icikt_k1plan.h and icikt_k0plan.h; here are the callers, which fill the context, talk to the
// device and print the verbose lines.  Declared in icikt_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::ColStats;
using icikt::PrepView;

namespace icikt {
namespace host {

int prepare_alloc(icikt_ctx* c, int64_t n_feat, int64_t n_samp, int64_t alloc_cols, int64_t sort_cols) {
  c->ref.valid = false;   // the tables are laid out anew: a prepared reference is gone
  c->prepared = false;
  c->raw_valid = false;
  PrepView pv{};
  pv.n = (int)n_feat;
  pv.n_pad = (int)((n_feat + 63) / 64 * 64);
  if (pv.n_pad == 0) pv.n_pad = 64;
  pv.n_ord = pv.n_pad + 256;  // K1 loads rows up to three steps ahead: indices up to n + 191, zero padded
  pv.rec_rows = pv.n_pad + 8;  // row n_pad: the guard row (PrepView::rec_rows)
  pv.W = (int)((n_feat + 63) / 64);
  pv.Wp = pv.W + 1;
  int np2 = 2;
  while (np2 < pv.n) np2 <<= 1;
  pv.npow2 = np2;
  pv.n_samp = (int)n_samp;
  const size_t S = (size_t)std::max<int64_t>(alloc_cols, 1);
  const size_t ncols = (size_t)std::max<int64_t>(sort_cols, 1);

  pv.wide = n_feat > ICIKT_MAX_FEATURES ? 1 : 0;
  pv.mstride = 3 * pv.Wp + (int)(sizeof(ColStats) / 8);
  HIPCHK(c, c->meta.reserve(S * (size_t)pv.mstride));
  pv.tg_stride = pv.n_pad / 2 + 1;
  // sort scratch: bounded to ~1 GiB
  size_t chunk = std::min<size_t>(ncols, std::max<size_t>(1, ((size_t)1 << 30) / ((size_t)np2 * 12)));
  if (pv.wide) {
    // 32-bit positions in four separate arrays; the 16-bit arrays of the tuned kernels are not needed
    HIPCHK(c, c->wide32.reserve(4 * S * (size_t)pv.n_pad));
    HIPCHK(c, c->k0_bits.reserve(chunk * 2 * (size_t)(pv.Wp + 1)));
    HIPCHK(c, c->order.reserve(1));
    HIPCHK(c, c->hirow.reserve(1));
    HIPCHK(c, c->girow.reserve(1));
    HIPCHK(c, c->rec.reserve(2));
    HIPCHK(c, c->tgroups.reserve(1));
    HIPCHK(c, c->tprog.reserve(1));
    HIPCHK(c, c->smask.reserve(1));
    HIPCHK(c, c->srow.reserve(1));
  } else {
    HIPCHK(c, c->order.reserve(S * pv.n_ord));
    HIPCHK(c, c->hirow.reserve(((S + 1) & ~(size_t)1) * pv.rec_rows));  // interleaved like rec: [S/2 blocks][rec_rows rows][2 columns]
    HIPCHK(c, c->girow.reserve(((S + 1) & ~(size_t)1) * pv.rec_rows));  // likewise
    HIPCHK(c, c->rec.reserve(((S + 1) & ~(size_t)1) * pv.rec_rows));  // [S/2 blocks][rec_rows rows][2 columns]
    HIPCHK(c, c->tgroups.reserve(S * (size_t)pv.tg_stride));
    // the tie program serves the half-wave kernels only (n <= 18 336); longer columns classify their steps in the pair kernel
    pv.tp_stride = (icikt::k1_half_items(pv.Wp) <= icikt::ICIKT_HALF_ITEMS_MAX) ? pv.n_pad + 2 : 0;
    HIPCHK(c, c->tprog.reserve(std::max<size_t>(1, S * (size_t)pv.tp_stride)));
    // a step's record (its rows in lane layout, a MIXED step's same-group masks); + 3 guard steps behind the last one
    pv.sr_steps = pv.tp_stride ? pv.n_pad / 17 + 8 : 0;
    HIPCHK(c, c->srow.reserve(std::max<size_t>(1, S * (size_t)pv.sr_steps * 64)));
    HIPCHK(c, c->smask.reserve(std::max<size_t>(1, S * (size_t)pv.sr_steps * 32)));
    if (pv.tp_stride == 0) HIPCHK(c, c->order_w.reserve(S * (size_t)pv.n_ord));   // (the whole-wave kernels' ring reload: PrepView::order_w)
  }
  HIPCHK(c, c->sort_keys.reserve(chunk * np2));
  HIPCHK(c, c->sort_idx.reserve(chunk * np2));
  c->sort_chunk = (int)chunk;

  pv.order = c->order.p; pv.hirow = c->hirow.p; pv.girow = c->girow.p; pv.rec = c->rec.p;
  pv.order_w = (!pv.wide && pv.tp_stride == 0) ? c->order_w.p : nullptr;
  pv.meta = c->meta.p;
  pv.sort_keys = c->sort_keys.p; pv.sort_idx = c->sort_idx.p;
  pv.tgroups = c->tgroups.p;
  pv.tprog = c->tprog.p;
  pv.srow = c->srow.p;
  pv.smask = c->smask.p;
  if (pv.wide) {
    pv.order32 = c->wide32.p;
    pv.q32 = pv.order32 + S * (size_t)pv.n_pad;
    pv.lo32 = pv.q32 + S * (size_t)pv.n_pad;
    pv.hi32 = pv.lo32 + S * (size_t)pv.n_pad;
    pv.k0_bits = c->k0_bits.p;
  }
  c->pv = pv;
  c->alloc_cols = (int64_t)S;
  return ICIKT_SUCCESS;
}

int mask_alloc(icikt_ctx* c, int64_t n_feat, int64_t n_samp) {
  c->ref.valid = false;
  c->prepared = false;
  c->raw_valid = false;
  PrepView pv{};
  pv.n = (int)n_feat;
  pv.n_pad = std::max(64, (int)((n_feat + 63) / 64 * 64));
  pv.W = (int)((n_feat + 63) / 64);
  pv.Wp = pv.W + 1;
  pv.n_samp = (int)n_samp;
  pv.mstride = pv.Wp;                      // the missing-row bitset is all a column's record holds here
  HIPCHK(c, c->meta.reserve((size_t)std::max<int64_t>(n_samp, 1) * (size_t)pv.mstride));
  pv.meta = c->meta.p;
  c->pv = pv;
  return ICIKT_SUCCESS;
}

int prepare_launch(icikt_ctx* c, const double* dX, int64_t ld, int64_t col_begin, int64_t col_end, hipStream_t stream) {
  const PrepView& pv = c->pv;
  if (!stream) stream = c->stream;
  c->raw_valid = false;
  c->tied_state = -1;
  c->ntg_hint = -1;
  c->group_hint = 0;
  if (col_end > col_begin)
    HIPCHK(c, hipMemsetAsync(c->meta.p + (size_t)col_begin * pv.mstride, 0,
                             (size_t)(col_end - col_begin) * pv.mstride * sizeof(unsigned long long), stream));
  if (pv.n > 0) {
    const int64_t chunk = std::max(1, c->sort_chunk);
    for (int64_t c0 = col_begin; c0 < col_end; c0 += chunk) {
      const int nc = (int)std::min<int64_t>(chunk, col_end - c0);
      const int shape = (c->k0_shape < 0 && c->k0_small) ? (int)K0_SHAPE_SMALL
                                                         : k0_launch_shape(c->k0_shape, pv.n, nc, c->prop.multiProcessorCount);
      if (c->plan_ov.verbose)
        fprintf(stderr, "[icikt] K0 plan: shape=%d (0 large, 1 small, 2 two per CU), %d rows x %d columns, %d CUs\n", shape, pv.n, nc,
                c->prop.multiProcessorCount);
      HIPCHK(c, icikt::launch_k0(pv, dX, ld, (int)c0, nc, c->k0_mask, c->k0_keep, shape, stream));
    }
  }
  return ICIKT_SUCCESS;
}

// The verdict on the prepared columns' tie structure (tie_verdict, icikt_k1plan.h), only asked where it chooses the kernel.
// The statistics of up to 64 columns are read back once per prepared matrix -- after `ready` (an event behind their
// pre-pass; nullptr: the context's stream) -- and the verdict is kept.
static bool matrix_tied(icikt_ctx* c, int64_t ncols_ready, hipEvent_t ready) {
  const PrepView& pv = c->pv;
  const int hi = icikt::k1_half_items(pv.Wp);
  const bool long_cols = hi > icikt::ICIKT_HALF_ITEMS_MAX;
  // (9 words per lane: the family is the half-wave one anyway; the read-back serves the size of the counter tables, plan_k1)
  if (pv.wide || hi < 9 || pv.n <= 0 || (!long_cols && c->plan_ov.half >= 0) || (long_cols && c->plan_ov.np > 0)) return false;
  if (c->tied_state >= 0) return c->tied_state != 0;
  const int64_t m = std::min<int64_t>(std::min<int64_t>(ncols_ready, pv.n_samp), 64);
  if (m <= 0) return false;
  const hipError_t es = ready ? hipEventSynchronize(ready) : hipStreamSynchronize(c->stream);
  if (es != hipSuccess) { (void)hipGetLastError(); return false; }
  std::vector<icikt::ColStats> st((size_t)m);
  if (hipMemcpy2D(st.data(), sizeof(icikt::ColStats), pv.col_stats(0), (size_t)pv.mstride * sizeof(unsigned long long),
                  sizeof(icikt::ColStats), (size_t)m, hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  const icikt::host::TieVerdict v = icikt::host::tie_verdict(st, pv.n, long_cols);
  c->tied_state = v.tied_state;
  c->ntg_hint = v.ntg_hint;
  c->group_hint = v.group_hint;
  if (c->plan_ov.verbose) fprintf(stderr, "[icikt] %lld columns read back: %.1f tie groups per column (at most %d), %.1f rows per group, a tied pair's group %d rows -> %s\n", (long long)m,
                                  (double)v.groups / (double)m, c->ntg_hint, (double)v.rows / (double)v.all_groups, c->group_hint,
                                  long_cols ? (c->tied_state ? "one pair per wave" : "two pairs per wave") : (c->tied_state ? "half-wave kernels" : "whole-wave kernels"));
  return c->tied_state != 0;
}

void settle_tie_verdict(icikt_ctx* c) { (void)matrix_tied(c, c->pv.n_samp, nullptr); }

// the host copies of a combn range (the device arrays were filled by a kernel)
static void ensure_host_pairs(icikt_ctx* c) {
  if (c->h_pairs_valid) return;
  icikt::host::combn_pairs(c->combn_S, c->combn_begin, c->combn_end, c->h_pi, c->h_pj);
  c->h_pairs_valid = true;
}

// the task list of the context's pair list (icikt_k1plan.h: build_units)
static void rebuild_units(icikt_ctx* c, int np) {
  ensure_host_pairs(c);
  icikt::host::build_units(c->h_pi, c->h_pj, c->n_pairs, np, c->h_units);
  c->n_units = (int)(c->h_units.size() / 2);
  c->wpb = np;
}

int upload_pairs(icikt_ctx* c) {
  const int64_t P = c->n_pairs;
  HIPCHK(c, c->d_pi.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, c->d_pj.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, c->d_raw.reserve((size_t)std::max<int64_t>(P, 1)));
  if (P > 0) {
    int rc = icikt::host::upload_sync(c, c->d_pi.p, c->h_pi.data(), (size_t)P * sizeof(int32_t));
    if (!rc) rc = icikt::host::upload_sync(c, c->d_pj.p, c->h_pj.data(), (size_t)P * sizeof(int32_t));
    if (rc) return rc;
  }
  return ICIKT_SUCCESS;
}

static int upload_units(icikt_ctx* c) {
  HIPCHK(c, c->d_unit_start.reserve(c->h_units.size()));
  return icikt::host::upload_sync(c, c->d_unit_start.p, c->h_units.data(), c->h_units.size() * sizeof(int32_t));
}

// One launch of the pair kernel over tasks [first, first + count) of the uploaded task list, on c->stream.
static int launch_pair_tasks(icikt_ctx* c, const K1Plan& pl, int first, int count) {
  if (count <= 0) return ICIKT_SUCCESS;
  int per_cu = 0;
  if (pl.half_items == 0) {
    HIPCHK(c, icikt::k1_blocks_per_cu(pl.np, pl.half_items, pl.wpb, pl.lds_bytes, &per_cu));
    if (per_cu < 1) per_cu = 1;
  }
  // (icikt_k1plan.h, k1_grid: which launches are cut in segments and which run persistent waves, and why)
  const icikt::host::K1Grid g = icikt::host::k1_grid(pl, count, per_cu, c->prop.multiProcessorCount, c->plan_ov.grid_mult, c->plan_ov.grid_cap);
  if (g.split > 1) HIPCHK(c, icikt::launch_zero_raw(c->d_unit_start.p + 2 * (size_t)first, count, c->d_raw.p, c->stream));
  if (g.persistent) {
    HIPCHK(c, c->d_task_ctr.reserve(8));
    HIPCHK(c, hipMemsetAsync(c->d_task_ctr.p, 0, 8 * sizeof(int), c->stream));
  }
  if (c->plan_ov.verbose)
    fprintf(stderr, "[icikt] K1 plan: np=%d half_items=%d wpb=%d lds=%zu B/block (%d B/pair, %d tie-group counters), %d blocks/CU x %d CUs, "
            "grid=%d%s, tasks=%d (from %d), %d segment(s) per task\n",
            pl.np, pl.half_items, pl.wpb, pl.lds_bytes, pl.perpair_bytes, icikt::k1_opt_cnt_cap(pl.opts), per_cu,
            c->prop.multiProcessorCount, g.blocks, g.persistent ? " (persistent)" : "", count, first, g.split);
  HIPCHK(c, icikt::launch_k1(c->pv, c->d_unit_start.p + 2 * (size_t)first, count, c->d_pi.p, c->d_pj.p, c->d_raw.p, pl.np,
                             pl.half_items, pl.wpb, g.blocks, pl.lds_bytes, pl.perpair_bytes,
                             g.persistent ? c->d_task_ctr.p : nullptr, g.opts, c->stream));
  return ICIKT_SUCCESS;
}

int run_counts(icikt_ctx* c, uint32_t flags) {
  int rc = ICIKT_SUCCESS;
  if (c->pv.wide) {
    // wide columns: the plain 32-bit pair kernel (one wave per pair, persistent single-wave workgroups that fetch
    // pairs from a counter)
    rc = timer_begin(c, ICIKT_K_PAIRS, flags);
    if (rc) return rc;
    const size_t lds = icikt::k1_wide_lds_bytes(c->pv.Wp);
    int per_cu = 0;
    HIPCHK(c, icikt::k1_wide_blocks_per_cu(lds, &per_cu));
    if (per_cu < 1) return fail(c, ICIKT_E_HIP, "run: the wide pair kernel does not fit a CU");
    const int blocks = (int)std::min<int64_t>(c->n_pairs, (int64_t)per_cu * c->prop.multiProcessorCount);
    HIPCHK(c, c->d_task_ctr.reserve(8));
    HIPCHK(c, hipMemsetAsync(c->d_task_ctr.p, 0, 8 * sizeof(int), c->stream));
    if (c->plan_ov.verbose)
      fprintf(stderr, "[icikt] K1 wide: lds=%zu B/wave, %d waves/CU, grid=%d, pairs=%lld\n", lds, per_cu, blocks,
              (long long)c->n_pairs);
    HIPCHK(c, icikt::launch_k1_wide(c->pv, c->d_pi.p, c->d_pj.p, c->d_raw.p, c->n_pairs, blocks, lds, c->d_task_ctr.p,
                                    c->stream));
  } else {
    const bool tied = matrix_tied(c, c->pv.n_samp, nullptr);
    const K1Plan pl = plan_k1(c->pv.n, c->pv.Wp, c->n_pairs, c->prop.multiProcessorCount, c->plan_ov, tied, c->ntg_hint, c->group_hint);
    if (c->wpb != pl.np) {
      rebuild_units(c, pl.np);
      c->units_dirty = true;
    }
    if (c->units_dirty) {
      rc = upload_units(c);
      if (rc) return rc;
      c->units_dirty = false;
    }
    rc = timer_begin(c, ICIKT_K_PAIRS, flags);
    if (rc) return rc;
    rc = launch_pair_tasks(c, pl, 0, c->n_units);
    if (rc) return rc;
  }
  rc = timer_end(c, ICIKT_K_PAIRS, flags);
  if (rc) return rc;
  c->raw_valid = true;
  return ICIKT_SUCCESS;
}

// H2D of columns [col_begin, col_end) + K0 over them.  The copies run on the context's copy stream in column
// chunks and K0 of a chunk waits only for its own chunk (an event per chunk), so the pre-pass of chunk i runs
// while chunk i + 1 crosses PCIe.  How the caller's matrix is read: MatrixUpload (icikt_transfer.h).
// prepass: kPrepassFull = K0; kPrepassMask = missing-row bitsets only (pairwise_completeness); kPrepassNone = the
// columns are only copied (icikt_pairs_complete_f64 sorts masked copies, not the columns).
// X is the caller's view of the whole matrix; a view that is not column-major float64 is widened / transposed on the
// device chunk by chunk (MatrixUpload::copy), so everything behind a chunk's event sees the same float64 columns.
int upload_and_prepare(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, int64_t col_begin,
                       int64_t col_end, uint32_t flags, bool pipelined, const std::function<int(size_t, int64_t)>* on_chunk,
                       int prepass) {
  // what runs over the columns of a chunk once they are on the device
  auto chunk_prepass = [&](int64_t c0, int64_t c1, hipStream_t st) -> int {
    if (prepass == kPrepassFull) return prepare_launch(c, c->d_X.p, n_feat, c0, c1, st);
    if (prepass == kPrepassMask) HIPCHK(c, icikt::launch_k0_mask(c->pv, c->d_X.p, n_feat, (int)c0, (int)(c1 - c0), st ? st : c->stream));
    return ICIKT_SUCCESS;
  };
  c->chunk_col_end.clear();
  c->xfer.csc_pending = false;
  // (X.dst_col > 0: the view is one of several sources of the device matrix and lands at that column; its caller has
  //  reserved d_X for all of them before the first upload -- a reserve that grows drops what the buffer holds)
  const int64_t at = X.dst_col;
  const size_t nel = (size_t)std::max<int64_t>(n_feat * (at + n_samp), 1);
  HIPCHK(c, c->d_X.reserve(nel));
  int rc = timer_begin(c, ICIKT_K_PREPARE, flags);
  if (rc) return rc;
  const int64_t ncols = col_end - col_begin;
  if (n_feat > 0 && ncols > 0) {
    // (icikt_k0plan.h: ~8 MB of columns, wider when pipelined or row-major, within the sort scratch)
    const int view = X.sparse ? K0_VIEW_SPARSE : X.v.order == ICIKT_ORDER_ROW ? K0_VIEW_ROW : K0_VIEW_COL;
    const int64_t chunk = k0_chunk_columns(n_feat, n_samp, c->prop.multiProcessorCount, pipelined, view,
                                           X.sparse ? sizeof(double) : dtype_bytes(X.v.dtype), prepass, c->sort_chunk);
    MatrixUpload up{c, X, n_feat, (!X.sparse && view_is_plain(X.v)) ? chunk : std::min<int64_t>(chunk, ncols)};
    size_t span = 0;
    if (X.sparse) {
      // the bytes the route is chosen by are the entries' (values + indices of the columns); the halves of the staging
      // blocks hold the chunk with the most entries
      up.n_samp = n_samp;
      for (int64_t c0 = col_begin; c0 < col_end; c0 += chunk)
        up.csc_max_nnz = std::max(up.csc_max_nnz, csc_ptr(X.s, std::min(c0 + chunk, col_end)) - csc_ptr(X.s, c0));
      span = (size_t)(csc_ptr(X.s, col_end) - csc_ptr(X.s, col_begin)) * (dtype_bytes(X.s.dtype) + index_bytes(X.s.index_type));
    } else {
      span = view_span(view_from_col(X.v, col_begin), n_feat, ncols);
    }
    hipError_t e = up.begin(span, pipelined ? c->prep_stream : nullptr);
    int k = 0;
    const int64_t first_chunk = chunk;   // (a short first chunk was measured twice: no gain -- what the last pair-kernel launch waits for is the last chunk's pre-pass, which finds no free CU until the launch before it drains)
    for (int64_t c0 = col_begin, step = first_chunk; c0 < col_end && e == hipSuccess && rc == 0; c0 += step, step = chunk, ++k) {
      const int64_t nc = std::min<int64_t>(step, col_end - c0);
      hipEvent_t ev = nullptr;
      e = up.copy(k, c->d_X.p + (size_t)(at + c0) * (size_t)n_feat, c0, nc, &ev);
      if (pipelined) {
        // the chunk's pre-pass on the pre-pass stream; an event of its own tells the pair kernel's stream when
        if (e == hipSuccess) e = hipStreamWaitEvent(c->prep_stream, ev, 0);
        // (Every chunk's pre-pass runs the 1 024-thread shape.  A workgroup of it needs an EMPTY CU, so a later chunk's
        //  pre-pass starts only when the pair-kernel launch in front of it drains -- round 3 put 0.5 ms of a c4 call down to
        //  that.  Round 4 built the 256-thread shape (k0_prepare_small: fits beside a running pair kernel, plan key k0=1) and
        //  measured it here: the pre-pass then does finish earlier, 3.9 against 6.4 ms into the call, but the call gets
        //  LONGER, 11.76 against 11.61 ms staged, 11.24 against 11.13 pinned (profiles/r04_ab_pipe_k0.log) -- both kernels
        //  are bound by vector issue, so overlapping them gains nothing, and the small shape takes 0.80 ms for the 1 024
        //  columns where the large one takes 0.65.)
        if (e == hipSuccess) rc = chunk_prepass(at + c0, at + c0 + nc, c->prep_stream);
        if ((size_t)k >= c->ev_chunk.size()) {
          hipEvent_t ne = nullptr;
          if (e == hipSuccess) e = hipEventCreateWithFlags(&ne, hipEventDisableTiming);
          if (e == hipSuccess) c->ev_chunk.push_back(ne);
        }
        if (e == hipSuccess && rc == 0) e = hipEventRecord(c->ev_chunk[(size_t)k], c->prep_stream);
        if (e == hipSuccess && rc == 0) c->chunk_col_end.push_back(c0 + nc);
        // the caller's work for this chunk (its pair-kernel launch) is enqueued NOW, before the host stages the next chunk
        if (e == hipSuccess && rc == 0 && on_chunk) rc = (*on_chunk)((size_t)k, c0 + nc);
      } else {
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev, 0);
        if (e == hipSuccess) rc = chunk_prepass(at + c0, at + c0 + nc, nullptr);
      }
    }
    if (e == hipSuccess && rc == 0) e = up.finish();   // (a CSC view: the scatter kernel's error record comes back behind the last chunk)
    if (pipelined && (e != hipSuccess || rc)) (void)hipStreamSynchronize(c->prep_stream);
    // The staging buffer serves the later transfers of the call as their bounce buffer, so its last copy is waited for
    // here.  A matrix the caller has page-locked is read in place: the pipelined callers go on with host work (the task
    // list) and wait for the copy stream themselves before they return (end_call) -- no entry point returns while
    // a copy still reads the caller's memory.
    const bool drained = !(pipelined && up.in_place) || e != hipSuccess || rc;
    if (drained) {
      const hipError_t es = hipStreamSynchronize(c->copy_stream);
      if (e == hipSuccess) e = es;
    }
    if (e != hipSuccess) { c->xfer.csc_pending = false; return fail(c, ICIKT_E_HIP, std::string("H2D of the matrix: ") + hipGetErrorString(e)); }
    if (rc) { c->xfer.csc_pending = false; return rc; }
    // malformed CSC input fails the call as soon as the copy stream has drained (else: end_call)
    if (drained) {
      rc = csc_verdict(c);
      if (rc) { if (pipelined) (void)hipStreamSynchronize(c->prep_stream); return rc; }
    }
  } else if (ncols > 0 && prepass == kPrepassFull) {
    rc = prepare_launch(c, c->d_X.p, n_feat, at + col_begin, at + col_end);  // n_feat == 0: statistics of empty columns
    if (rc) return rc;
  }
  return timer_end(c, ICIKT_K_PREPARE, flags);
}

// The pair kernel's task list for the prepared shape and the current pair list, built on the host now (while
// copies and the pre-pass run) instead of inside icikt_run_dev, which then only uploads it.
void prebuild_units(icikt_ctx* c) {
  if (c->n_pairs <= 0 || c->pv.wide) return;
  const K1Plan pl = plan_k1(c->pv.n, c->pv.Wp, c->n_pairs, c->prop.multiProcessorCount, c->plan_ov, false);   // (icikt_run_dev rebuilds the list if the columns' tie structure asks for another np)
  if (c->wpb != pl.np) {
    rebuild_units(c, pl.np);
    c->units_dirty = true;
  }
}

// The host entries' H2D + pre-pass + pair kernel.  A matrix of several 8 MB chunks is PIPELINED: all copies and all
// pre-pass launches are enqueued at once (copy stream -> pre-pass stream, an event per chunk); meanwhile the host
// builds the task list, orders it by the chunk in which a task's LAST column arrives, and enqueues one pair-kernel
// launch per chunk behind that chunk's pre-pass event.  The pairs among the columns that have arrived are counted
// while the rest of the matrix still crosses PCIe: the available work grows with the square of the arrived columns,
// so after the first millisecond of a c4-sized call the GPU never waits for the link again.
int upload_prepare_pairs(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, uint32_t flags) {
  const size_t col_bytes = (size_t)n_feat * sizeof(double);
  // (the size that decides for the pipeline is the float64 matrix's, whatever the view's element type and order: a view
  //  runs the launches its float64 copy runs)
  const int64_t ld = (!X.sparse && view_is_plain(X.v)) ? X.v.ld : n_feat;
  const size_t span = (n_samp > 0 && n_feat > 0) ? ((size_t)(n_samp - 1) * (size_t)ld + (size_t)n_feat) * sizeof(double) : 0;
  const bool can = !c->pv.wide && n_feat > 0 && c->n_pairs > 0;
  const bool want = c->pipe_mode < 0 ? (span >= ((size_t)24 << 20)) : (c->pipe_mode == 1 && (size_t)n_samp * col_bytes > ((size_t)8 << 20));
  // A pair list that does not fill the chip several times: copies and pre-pass stay pipelined by chunks, but the pairs run in
  // ONE launch behind the last chunk's pre-pass -- a launch of a few thousand tasks lasts as long as one task whatever its
  // size, and a launch per chunk puts those latencies one behind the other (50 000 x 96 tied columns: 15.5 -> 9.5 ms)
  const bool merge_launches = c->plan_ov.merge >= 0 ? c->plan_ov.merge != 0 : c->n_pairs < (int64_t)4 * 48 * c->prop.multiProcessorCount;
  if (!(can && want)) {
    int rc = upload_and_prepare(c, X, n_feat, n_samp, 0, n_samp, flags);
    if (rc) return rc;
    c->prepared = true;
    prebuild_units(c);   // host work under the copies; icikt_run_dev uploads the list
    return ICIKT_SUCCESS;   // (the caller's icikt_run_dev runs the pair kernel)
  }
  const auto t0 = std::chrono::steady_clock::now();
  auto ms_since = [&t0]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  K1Plan pl = plan_k1(c->pv.n, c->pv.Wp, c->n_pairs, c->prop.multiProcessorCount, c->plan_ov, false);
  const bool all_combn = c->combn_S == n_samp && c->combn_begin == 0 && c->combn_end == n_samp * (n_samp - 1) / 2;
  double t_enq = 0, t_built = 0, t_up = 0;

  // ---- the steps both producers of task slices share ----
  // (18 337 .. 30 656 rows: the first chunk's columns say which kernel family runs; both take two pairs per task)
  auto replan = [&](int64_t cols_ready) {
    const bool tied = matrix_tied(c, cols_ready, c->ev_chunk[0]);
    if (tied || c->ntg_hint >= 0) pl = plan_k1(c->pv.n, c->pv.Wp, c->n_pairs, c->prop.multiProcessorCount, c->plan_ov, tied, c->ntg_hint, c->group_hint);
  };
  // The launch of chunk q, which brought the columns up to ce and whose tasks are [first_q, end_q) of the device list,
  // behind that chunk's pre-pass event; staged: the list's pinned host copy, of which the launch's slice is uploaded
  // first (nullptr: the list is on the device already).  merge_launches: nothing until the last chunk, then the whole list.
  // (the launches stay on ONE stream: alternating consecutive chunks' launches between two streams, so that one starts
  //  while the other drains, was measured slower -- 12.3 against 11.6 ms on c4, round 4: two launches in flight share
  //  the SIMDs and the cache with the small-shape pre-pass and each other)
  auto launch_chunk = [&](size_t q, int64_t ce, size_t first_q, size_t end_q, const int32_t* staged) -> int {
    if (merge_launches && ce < n_samp) return ICIKT_SUCCESS;
    const size_t first = merge_launches ? 0 : first_q, cnt = end_q - first;
    if (staged && cnt == 0) return ICIKT_SUCCESS;
    hipError_t e = hipSuccess;
    if (staged) e = hipMemcpyAsync(c->d_unit_start.p + 2 * first, staged + 2 * first, cnt * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->ev_chunk[q], 0);
    if (e != hipSuccess) return fail(c, ICIKT_E_HIP, std::string("pipelined pairs: ") + hipGetErrorString(e));
    return launch_pair_tasks(c, pl, (int)first, (int)cnt);
  };

  int rc = ICIKT_SUCCESS;
  if (all_combn) {
    // All pairs of the upper triangle: a chunk's tasks are arithmetic (combn_chunk_units).  They are written chunk by
    // chunk straight into a pinned buffer, copied asynchronously and launched AS SOON AS the chunk's copy and pre-pass
    // are enqueued (the callback below runs inside upload_and_prepare's chunk loop: with staged transfers the host is
    // busy copying the next chunk into its pinned buffer meanwhile) -- the first launch is enqueued a fraction of a
    // millisecond into the call, no host copy of the pair list is ever made.
    const size_t cap_tasks = (size_t)c->n_pairs + (size_t)n_samp + 8;
    HIPCHK(c, c->d_unit_start.reserve(cap_tasks * 2));
    int32_t* u = nullptr;
    rc = task_staging(c, cap_tasks * 2, &u);
    if (rc) return rc;
    size_t nt = 0;
    int64_t cb = 0;
    const std::function<int(size_t, int64_t)> on_chunk = [&](size_t q, int64_t ce) -> int {
      if (q == 0) replan(ce);
      const size_t first_q = nt;
      nt += combn_chunk_units(n_samp, cb, ce, pl.np, u + 2 * nt);
      cb = ce;
      return launch_chunk(q, ce, first_q, nt, u);
    };
    rc = timer_begin(c, ICIKT_K_PAIRS, flags);
    if (rc == 0) rc = upload_and_prepare(c, X, n_feat, n_samp, 0, n_samp, flags & ~ICIKT_FLAG_TIMING, true, &on_chunk);
    if (rc == 0) {
      c->prepared = true;
      c->n_units = (int)nt;
      c->wpb = 0;               // (h_units does not hold this list: a later device-resident run rebuilds it)
      c->units_dirty = true;
      t_enq = t_built = t_up = ms_since();
    }
  } else {
    // Any other pair list: everything is enqueued first, the task list is built while the copies run (build_units),
    // ordered by the chunk of a task's last column (order_units_by_chunk) and uploaded whole, then launched chunk by chunk.
    rc = upload_and_prepare(c, X, n_feat, n_samp, 0, n_samp, flags & ~ICIKT_FLAG_TIMING, true, nullptr);
    const size_t nchunks = c->chunk_col_end.size();
    std::vector<int> first;
    if (rc == 0) {
      c->prepared = true;
      t_enq = ms_since();
      if (nchunks > 0) replan(c->chunk_col_end[0]);
      rebuild_units(c, pl.np);
      order_units_by_chunk(c->h_units, c->h_pi.data(), c->h_pj.data(), c->chunk_col_end, first);
      t_built = ms_since();
      rc = upload_units(c);
    }
    if (rc == 0) {
      c->units_dirty = false;
      t_up = ms_since();
      rc = timer_begin(c, ICIKT_K_PAIRS, flags);
    }
    for (size_t q = 0; q < nchunks && rc == 0; ++q)
      rc = launch_chunk(q, c->chunk_col_end[q], (size_t)first[q], (size_t)first[q + 1], nullptr);
  }
  if (rc == 0) rc = timer_end(c, ICIKT_K_PAIRS, flags);
  if (rc) { (void)hipStreamSynchronize(c->prep_stream); return rc; }   // the one way out on an error: the pre-pass stream drained
  c->raw_valid = true;
  if (c->plan_ov.verbose) {
    const double t_launched = ms_since();
    (void)hipStreamSynchronize(c->copy_stream);
    const double t_copied = ms_since();
    (void)hipStreamSynchronize(c->prep_stream);
    const double t_prepped = ms_since();
    (void)hipStreamSynchronize(c->stream);
    fprintf(stderr, "[icikt] pipelined: %zu chunks; enqueued copies + pre-pass %.2f ms, tasks built %.2f, uploaded %.2f, pair launches "
                    "enqueued %.2f, copies done %.2f, pre-pass done %.2f, pairs done %.2f ms\n", c->chunk_col_end.size(), t_enq, t_built, t_up,
            t_launched, t_copied, t_prepped, ms_since());
  }
  return ICIKT_SUCCESS;
}

}  // namespace host
}  // namespace icikt
