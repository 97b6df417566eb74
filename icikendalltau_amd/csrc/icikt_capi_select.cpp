// icikt_capi_select.cpp -- the host side the ten selection entries share (icikt_topk_*, icikt_edges_*,
// icikt_class_medians_*, icikt_class_matrix_*, icikt_quantiles_*, icikt_padjust_*, icikt_mst_*, icikt_anosim_*,
// icikt_hclust_*, icikt_permanova_*; declared in icikt_host.h) and icikt_cross_* runs its rectangle through: their common checks, the run of a call's blocks through the pair engine,
// and the steps several of them take over the one set of key planes (icikt_ctx::sel) -- the fold that keeps a block's
// raw as keys, the radix sort, the download of d_red -- and, for the two permutation tests, the check of the class
// labels and the batches of labellings (select_labellings).  The driver allocates nothing of size S^2: each block's
// records are folded by the entry's kernel before the next block overwrites them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

namespace icikt {
namespace host {

int select_check_shape(const SelectCall& s, const char* cap_why) {
  if (!s.c) return ICIKT_E_INVALID;
  const int rc = check_src(s.c, s.who, s.X, s.n_feat, s.n_samp);
  if (rc) return rc;
  if (s.n_samp > ICIKT_TOPK_MAX_SAMPLES)
    return fail(s.c, ICIKT_E_INVALID, std::string(s.who) + ": n_samp exceeds ICIKT_TOPK_MAX_SAMPLES (65535 samples: " + cap_why + ")");
  return ICIKT_SUCCESS;
}

int select_check_args(SelectCall& s) {
  const SelectArgs& A = s.A;
  if (A.perspective != ICIKT_PERSPECTIVE_LOCAL && A.perspective != ICIKT_PERSPECTIVE_GLOBAL)
    return fail(s.c, ICIKT_E_INVALID, std::string(s.who) + ": perspective must be local (0) or global (1)");
  if (A.alternative < 0 || A.alternative > ICIKT_ALT_OTHER)
    return fail(s.c, ICIKT_E_INVALID, std::string(s.who) + ": bad alternative code");
  const int rc = make_mask_spec(s.c, A.global_na, A.n_global_na, &s.ms);
  if (rc) return rc;
  if (A.reason_counts) for (int r = 0; r < 5; ++r) A.reason_counts[r] = 0;
  if (A.max_taumax) *A.max_taumax = -HUGE_VAL;   // max(numeric(0), na.rm = TRUE)
  return ICIKT_SUCCESS;
}

int select_budget(const SelectCall& s, int64_t* budget) {
  *budget = s.c->plan_ov.tkblock > 0 ? s.c->plan_ov.tkblock : kTriangleBlockPairs;
  return use_device(s.c);
}

int select_run(SelectCall& s, PairBlocks& blocks, const SelectSteps& steps) {
  icikt_ctx* const c = s.c;
  const SelectArgs& A = s.A;
  const uint32_t flags = A.flags;
  HIPCHK(c, c->d_red.reserve(8));
  // from here on the context holds this call's scratch state and nothing of the caller's: whatever happens, the
  // device-resident calls start over afterwards (icikt_run_dev: ICIKT_E_STATE, icikt_num_pairs: -1)
  auto leave = [&](int r) {
    r = end_call(c, s.who, r);
    forget_prepared(c);
    return r;
  };
  const PinnedScope scope(c, flags);
  const uint32_t run_flags = flags & ~(uint32_t)ICIKT_FLAG_REUSE_COUNTS;
  unsigned long long red[8] = {};
  auto body = [&]() -> int {
    int r = steps.start();
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->d_red.p, 0, 8 * sizeof(unsigned long long), c->stream));
    if (blocks.n_blocks > 0) {
      HIPCHK(c, c->d_out4.reserve((size_t)blocks.block_max * 4));
      HIPCHK(c, c->d_reasons.reserve((size_t)blocks.block_max));
      PairBlock b;
      bool more = false;
      auto advance = [&]() -> int {
        try { more = blocks.next(&b); } catch (const std::bad_alloc&) {
          return fail(c, ICIKT_E_NOMEM, std::string(s.who) + ": host allocation failed");
        }
        return ICIKT_SUCCESS;
      };
      auto set_pairs = [&]() {
        return b.pi ? icikt_set_pairs(c, b.pi, b.pj, b.count) : icikt_set_pairs_combn(c, blocks.S, b.begin, b.begin + b.count);
      };
      // a call that is one block takes the matrix entries' way in: copies, pre-pass and pair kernel pipelined by
      // column chunks (upload_prepare_pairs); several blocks: the matrix first, then block after block
      // (an entry with an upload step of its own brings the matrix first and takes the second way)
      const bool one = blocks.n_blocks == 1 && !steps.upload;
      r = advance();
      if (!r && one) r = set_pairs();
      if (r) return r;
      if (steps.upload) {
        r = steps.upload();
      } else {
        r = prepare_alloc(c, s.n_feat, s.n_samp, s.n_samp, s.n_samp);
        if (r) return r;
        c->k0_mask = &s.ms;
        c->k0_keep = nullptr;
        r = one ? upload_prepare_pairs(c, s.X, s.n_feat, s.n_samp, flags)
                : upload_and_prepare(c, s.X, s.n_feat, s.n_samp, 0, s.n_samp, flags);
      }
      c->k0_mask = nullptr;
      if (r) return r;
      c->prepared = true;
      int64_t done = 0;
      while (more) {
        if (!one) {
          r = set_pairs();
          if (r) return r;
        }
        if (b.count <= 0 || b.begin != done || done + b.count > blocks.total)
          return fail(c, ICIKT_E_STATE, std::string(s.who) + ": the block cut lost its place");
        r = icikt_run_dev(c, A.perspective, A.alternative, A.continuity,
                          run_flags | ((one && c->raw_valid) ? ICIKT_FLAG_REUSE_COUNTS : 0u), c->d_out4.p, nullptr,
                          c->d_reasons.p);
        if (r) return r;
        r = timer_begin(c, ICIKT_K_EPILOGUE, flags);
        if (r) return r;
        HIPCHK(c, launch_out_stats_accum(c->pv, c->d_out4.p, c->d_reasons.p, b.count, c->d_red.p, c->stream));
        r = steps.fold(b);
        if (r) return r;
        r = timer_end(c, ICIKT_K_EPILOGUE, flags);
        if (r) return r;
        done += b.count;
        r = advance();
        if (r) return r;
      }
      if (done != blocks.total) return fail(c, ICIKT_E_STATE, std::string(s.who) + ": the blocks do not add up to the pair list");
    }
    return steps.finish(red);
  };
  const int rc = leave(body());
  c->k0_mask = nullptr;
  if (rc) return rc;
  // d_red: word 0 the largest taumax as an order-preserving key (0: no pair had one), words 1 .. 5 the reason counts
  if (A.reason_counts) for (int r = 0; r < 5; ++r) A.reason_counts[r] = (int64_t)red[1 + r];
  if (A.max_taumax) *A.max_taumax = max_taumax_of(red[0]);
  return ICIKT_SUCCESS;
}

int select_keep_raw(icikt_ctx* c, const PairBlock& b) {
  HIPCHK(c, launch_median_keep(c->d_out4.p, c->d_reasons.p, b.count, c->sel.kept.p + b.begin, c->stream));
  return ICIKT_SUCCESS;
}

int select_download_red(icikt_ctx* c, unsigned long long* red) {
  return download(c, red, c->d_red.p, 8 * sizeof(unsigned long long));
}

int select_sort(icikt_ctx* c, int64_t P, long long tile, const unsigned long long* h_dhist, unsigned long long* a,
                unsigned long long* b, unsigned long long** sorted, unsigned long long** spare) {
  const long long n_tiles = (P + tile - 1) / tile;
  HIPCHK(c, c->sel.counts.reserve((size_t)std::max<long long>(256 * n_tiles, 1)));
  HIPCHK(c, c->sel.agg.reserve((size_t)padj_scan_chunks(P, tile)));
  for (int d = 0; d < 8; ++d) {
    bool same = false;   // one digit value holds all P keys: the pass would move nothing
    for (int v = 0; v < 256; ++v) same = same || h_dhist[d * 256 + v] == (unsigned long long)P;
    if (same) continue;
    HIPCHK(c, launch_padj_sort_pass(a, b, P, tile, 8 * d, c->sel.counts.p, c->sel.agg.p, c->stream));
    std::swap(a, b);
  }
  *sorted = a;
  *spare = b;
  return ICIKT_SUCCESS;
}

static_assert(ICIKT_ANOSIM_MAX_PERM == 1000000 && ICIKT_PERMANOVA_MAX_CELLS == 67108864, "the messages below spell the header's limits out");

static int bad_label(icikt_ctx* c, const char* who, const std::string& name, int64_t s, int32_t v, int64_t n_class) {
  return fail(c, ICIKT_E_INVALID, std::string(who) + ": " + name + "[" + std::to_string(s) + "] = " + std::to_string(v) +
                                      " is outside 0 .. n_class - 1 (n_class = " + std::to_string(n_class) + ")");
}

int check_labels(icikt_ctx* c, const char* who, const std::string& name, const int32_t* lab, int64_t n, int64_t n_class) {
  const int64_t s = first_bad_label(lab, n, n_class);
  return s < n ? bad_label(c, who, name, s, lab[s], n_class) : ICIKT_SUCCESS;
}

int select_check_classes(const SelectCall& s, const int32_t* cls, int n_class, int class_cap, const char* cap_why) {
  if (!cls) return ICIKT_SUCCESS;
  if (n_class < 1) return fail(s.c, ICIKT_E_INVALID, std::string(s.who) + ": n_class must be at least 1");
  if (class_cap > 0 && n_class > class_cap)
    return fail(s.c, ICIKT_E_INVALID, std::string(s.who) + ": n_class exceeds " + std::to_string(class_cap) + " (" + cap_why + ")");
  return check_labels(s.c, s.who, "cls", cls, s.n_samp, n_class);
}

int select_check_labellings(const SelectCall& s, const int32_t* cls, int n_class, int class_cap, const char* cap_why,
                            const int32_t* perm_cls, int64_t n_perm, int64_t cell_cap) {
  const int rc = select_check_classes(s, cls, n_class, class_cap, cap_why);
  if (rc) return rc;
  const std::string who = s.who;
  if (n_perm < 0) return fail(s.c, ICIKT_E_INVALID, who + ": n_perm must not be negative");
  if (n_perm > ICIKT_ANOSIM_MAX_PERM) return fail(s.c, ICIKT_E_INVALID, who + ": n_perm exceeds ICIKT_ANOSIM_MAX_PERM (1000000)");
  if (cell_cap > 0 && (1 + n_perm) * (int64_t)(cls ? n_class : 1) > cell_cap)
    return fail(s.c, ICIKT_E_INVALID, who + ": (1 + n_perm) n_class exceeds ICIKT_PERMANOVA_MAX_CELLS (67108864)");
  if (n_perm > 0 && !perm_cls) return fail(s.c, ICIKT_E_INVALID, who + ": null perm_cls with n_perm > 0");
  return ICIKT_SUCCESS;
}

int select_labellings_begin(const SelectCall& s, const int32_t* cls, int n_class, const int32_t* perm_cls, int64_t n_perm,
                            int64_t bytes_per_lab, Labellings* L) {
  L->perm_cls = perm_cls;
  L->S = s.n_samp;
  L->n_class = cls ? n_class : 1;   // a null cls: one class, n_class ignored
  L->n_lab = 1 + n_perm;            // the observed labelling, then the permutations
  L->plan = label_batches(L->S, L->n_lab, bytes_per_lab, s.c->plan_ov.anoperms);
  try {
    L->stage.assign(L->plan.stage_words, 0);
    L->obs.assign((size_t)L->S, 0);
    if (cls) std::copy(cls, cls + L->S, L->obs.begin());
    L->size_of.assign((size_t)L->n_class, 0);
  } catch (const std::bad_alloc&) {
    return fail(s.c, ICIKT_E_NOMEM, std::string(s.who) + ": host allocation failed");
  }
  HIPCHK(s.c, s.c->labels.reserve(L->plan.stage_words));
  return ICIKT_SUCCESS;
}

int select_labellings(const SelectCall& s, Labellings& L, bool device, int64_t* within, const LabellingSteps& steps) {
  icikt_ctx* const c = s.c;
  constexpr int PB = ANO_PB;
  int64_t in_flight = -1, in_flight_n = 0;   // first labelling and count of the batch whose kernels have been launched
  auto collect = [&]() -> int {
    if (in_flight < 0) return ICIKT_SUCCESS;
    const int64_t q0 = in_flight;
    in_flight = -1;
    return steps.collect(q0, in_flight_n);
  };
  for (int64_t q0 = 0; q0 < L.n_lab; q0 += L.plan.batch) {
    const int64_t nb = std::min<int64_t>(L.plan.batch, L.n_lab - q0);
    const int64_t groups = (nb + PB - 1) / PB;
    // (a collect reads the sums of the batch before, not the labels: the stage may be refilled while its kernels run,
    // the upload below is what waits for them)
    const BadLabel bad = stage_labellings(L.obs.data(), L.perm_cls, L.S, L.n_class, q0, nb, L.stage.data(),
                                          within ? within + q0 : nullptr, L.size_of.data());
    if (bad.q >= 0) return bad_label(c, s.who, "perm_cls[" + std::to_string(bad.q - 1) + "]", bad.s, bad.value, L.n_class);
    int r = collect();
    if (r) return r;
    if (!device) continue;
    r = upload_sync(c, c->labels.p, L.stage.data(), (size_t)groups * (size_t)L.S * PB * sizeof(uint16_t));
    if (!r) r = timer_begin(c, ICIKT_K_EPILOGUE, s.A.flags);
    if (r) return r;
    r = steps.launch(groups, nb);
    if (r) return r;
    r = timer_end(c, ICIKT_K_EPILOGUE, s.A.flags);
    if (r) return r;
    in_flight = q0;
    in_flight_n = nb;
  }
  return collect();
}

}  // namespace host
}  // namespace icikt
