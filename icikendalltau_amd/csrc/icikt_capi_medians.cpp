// icikt_capi_medians.cpp -- host side of icikt_class_medians_f64 / _in / _csc: every sample's median ICI-Kendall-tau
// over the other samples of its class, reduced on the device (icikt_medians.hip).  Only the within-class pairs run
// through the pair engine, in blocks; each block's raw values are kept as sortable keys (8 bytes per pair) before the
// next block overwrites them, and the select kernel reads the kept plane once the last block is through.
//
// Device memory: the prepared matrix, one block's buffers (icikt_host.h: kTriangleBlockPairs), 8 P bytes of kept keys
// for the P = sum over the classes of m (m - 1) / 2 computed pairs (one class of 65 535 samples: 17 GB) and 36 S bytes:
// the index arrays (position in class, class size, the class's first pair as int64: 16) and the results (20), each
// with the buffers' growth margin of a ninth.  Host memory: O(S) for the classes and O(block) for a slice's pi / pj, never O(P).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::timer_begin;
using icikt::host::timer_end;

using icikt::host::cut_rows;
using icikt::host::row_offset;

namespace {

// the members of the classes, class by class in class-index order, ascending sample index inside a class
struct ClassRuns {
  std::vector<int32_t> member;                  // [S] sample indices
  std::vector<std::pair<int32_t, int32_t>> run; // per non-empty class: [first, last) of `member`
};

// the pairs of the call's order from a cursor on: class `ci`, pair (a, b) of its members
struct PairCursor {
  size_t ci = 0;
  int32_t a = 0, b = 1;
};

// up to `budget` pairs from the cursor on into pi / pj (sample indices); the cursor moves behind them
void next_slice(const ClassRuns& cr, PairCursor* cur, int64_t budget, std::vector<int32_t>* pi, std::vector<int32_t>* pj) {
  pi->clear();
  pj->clear();
  while (cur->ci < cr.run.size() && (int64_t)pi->size() < budget) {
    const int32_t first = cr.run[cur->ci].first, m = cr.run[cur->ci].second - first;
    if (cur->a >= m - 1) {   // the class is through (a singleton has no pair)
      ++cur->ci;
      cur->a = 0;
      cur->b = 1;
      continue;
    }
    const int64_t take = std::min<int64_t>(m - cur->b, budget - (int64_t)pi->size());
    const int32_t sa = cr.member[first + cur->a];
    for (int64_t q = 0; q < take; ++q) {
      pi->push_back(sa);
      pj->push_back(cr.member[first + cur->b + q]);
    }
    cur->b += (int32_t)take;
    if (cur->b >= m) {
      ++cur->a;
      cur->b = cur->a + 1;
    }
  }
}

// the body of the three entries
int medians_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na,
                int n_global_na, const int32_t* cls, int n_class, int perspective, int alternative, int continuity,
                uint32_t flags, int scale_max, double* med2, int32_t* n_valid, double* max_taumax,
                int64_t* reason_counts) {
  if (!c) return ICIKT_E_INVALID;
  // every argument is validated before anything of the context or an output is touched
  int rc = icikt::host::check_src(c, "class_medians", X, n_feat, n_samp);
  if (rc) return rc;
  if (n_samp > ICIKT_TOPK_MAX_SAMPLES)
    return fail(c, ICIKT_E_INVALID, "class_medians: n_samp exceeds ICIKT_TOPK_MAX_SAMPLES (65535 samples: a class's pairs are indexed from 32-bit positions)");
  if (cls && n_class < 1) return fail(c, ICIKT_E_INVALID, "class_medians: n_class must be at least 1");
  if (cls)
    for (int64_t s = 0; s < n_samp; ++s)
      if (cls[s] < 0 || cls[s] >= n_class)
        return fail(c, ICIKT_E_INVALID, "class_medians: cls[" + std::to_string(s) + "] = " + std::to_string(cls[s]) +
                                            " is outside 0 .. n_class - 1 (n_class = " + std::to_string(n_class) + ")");
  if (n_samp > 0 && !med2) return fail(c, ICIKT_E_INVALID, "class_medians: null output (med2)");
  if (perspective != ICIKT_PERSPECTIVE_LOCAL && perspective != ICIKT_PERSPECTIVE_GLOBAL)
    return fail(c, ICIKT_E_INVALID, "class_medians: perspective must be local (0) or global (1)");
  if (alternative < 0 || alternative > ICIKT_ALT_OTHER) return fail(c, ICIKT_E_INVALID, "class_medians: bad alternative code");
  icikt::MaskSpec ms;
  rc = icikt::host::make_mask_spec(c, global_na, n_global_na, &ms);
  if (rc) return rc;
  if (reason_counts) for (int r = 0; r < 5; ++r) reason_counts[r] = 0;
  if (max_taumax) *max_taumax = -HUGE_VAL;   // max(numeric(0), na.rm = TRUE)
  if (n_samp == 0) return ICIKT_SUCCESS;
  rc = icikt::host::use_device(c);
  if (rc) return rc;

  // the classes: O(S) on the host, whatever n_class is
  const int64_t S = n_samp;
  ClassRuns cr;
  std::vector<int32_t> h_pos, h_size;
  std::vector<long long> h_base;
  int64_t total = 0;
  try {
    cr.member.resize((size_t)S);
    std::iota(cr.member.begin(), cr.member.end(), 0);
    if (cls) std::stable_sort(cr.member.begin(), cr.member.end(), [cls](int32_t a, int32_t b) { return cls[a] < cls[b]; });
    h_pos.resize((size_t)S);
    h_size.resize((size_t)S);
    h_base.resize((size_t)S);
    for (int64_t f = 0; f < S;) {
      int64_t l = f + 1;
      while (cls && l < S && cls[cr.member[l]] == cls[cr.member[f]]) ++l;
      if (!cls) l = S;
      cr.run.emplace_back((int32_t)f, (int32_t)l);
      const int64_t m = l - f;
      for (int64_t q = f; q < l; ++q) {
        const int32_t s = cr.member[q];
        h_pos[s] = (int32_t)(q - f);
        h_size[s] = (int32_t)m;
        h_base[s] = (long long)total;
      }
      total += m * (m - 1) / 2;
      f = l;
    }
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "class_medians: host allocation failed");
  }
  const bool one_class = cr.run.size() == 1;   // (all samples in it: the combn triangle)
  int64_t budget = c->plan_ov.tkblock > 0 ? c->plan_ov.tkblock : icikt::host::kTriangleBlockPairs;
  // one class: blocks of whole combn rows; several: slices of the explicit list (a pair list holds fewer than 2^31 - 1)
  std::vector<std::pair<int, int>> blocks;
  int64_t block_max = 1, n_slices = 0;
  if (one_class) {
    blocks = cut_rows(S, budget);
    for (const auto& b : blocks) block_max = std::max(block_max, row_offset(S, b.second) - row_offset(S, b.first));
  } else {
    budget = std::min<int64_t>(budget, (int64_t)1 << 30);
    n_slices = (total + budget - 1) / budget;
    block_max = std::max<int64_t>(1, std::min(total, budget));
  }
  const int stage = c->plan_ov.medlds >= 0 ? c->plan_ov.medlds : icikt::MEDIAN_STAGE_MAX;

  auto& md = c->med;
  HIPCHK(c, md.kept.reserve((size_t)std::max<int64_t>(total, 1)));
  HIPCHK(c, md.pos.reserve((size_t)S));
  HIPCHK(c, md.size.reserve((size_t)S));
  HIPCHK(c, md.base.reserve((size_t)S));
  HIPCHK(c, md.med2.reserve(2 * (size_t)S));
  HIPCHK(c, md.n_valid.reserve((size_t)S));
  HIPCHK(c, c->d_red.reserve(8));
  const icikt::MedianClasses mc{md.pos.p, md.size.p, md.base.p};

  // from here on the context holds this call's scratch state and nothing of the caller's: whatever happens, the
  // device-resident calls start over afterwards (icikt_run_dev: ICIKT_E_STATE, icikt_num_pairs: -1)
  auto leave = [c](int r) {
    r = icikt::host::end_call(c, "class_medians", r);
    c->prepared = false;
    c->raw_valid = false;
    c->n_pairs = -1;
    c->pairs_nsamp = -1;
    c->wpb = 0;
    c->combn_S = -1;
    return r;
  };
  const icikt::host::PinnedScope scope(c, flags);
  const uint32_t run_flags = flags & ~(uint32_t)ICIKT_FLAG_REUSE_COUNTS;
  unsigned long long red[8] = {};
  // a block's pairs are through the pair engine: their statistics and their keys, before the next block overwrites them
  auto fold = [&](int64_t begin, int64_t count) -> int {
    int r = timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_out_stats_accum(c->pv, c->d_out4.p, c->d_reasons.p, count, c->d_red.p, c->stream));
    HIPCHK(c, icikt::launch_median_keep(c->d_out4.p, c->d_reasons.p, count, md.kept.p + begin, c->stream));
    return timer_end(c, ICIKT_K_EPILOGUE, flags);
  };
  auto body = [&]() -> int {
    int r = icikt::host::upload_sync(c, md.pos.p, h_pos.data(), (size_t)S * sizeof(int32_t));
    if (!r) r = icikt::host::upload_sync(c, md.size.p, h_size.data(), (size_t)S * sizeof(int32_t));
    if (!r) r = icikt::host::upload_sync(c, md.base.p, h_base.data(), (size_t)S * sizeof(long long));
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->d_red.p, 0, 8 * sizeof(unsigned long long), c->stream));
    if (total > 0) {
      HIPCHK(c, c->d_out4.reserve((size_t)block_max * 4));
      HIPCHK(c, c->d_reasons.reserve((size_t)block_max));
      // a pair list that is one block takes the matrix entries' way in: copies, pre-pass and pair kernel pipelined by
      // column chunks (upload_prepare_pairs); several blocks: the matrix first, then block after block
      const bool one = one_class ? blocks.size() == 1 : n_slices == 1;
      std::vector<int32_t> pi, pj;
      PairCursor cur;
      if (one) {
        if (one_class) {
          r = icikt_set_pairs_combn(c, S, 0, total);
        } else {
          try { next_slice(cr, &cur, budget, &pi, &pj); } catch (const std::bad_alloc&) {
            return fail(c, ICIKT_E_NOMEM, "class_medians: host allocation failed");
          }
          r = icikt_set_pairs(c, pi.data(), pj.data(), (int64_t)pi.size());
        }
        if (r) return r;
      }
      r = icikt::host::prepare_alloc(c, n_feat, n_samp, n_samp, n_samp);
      if (r) return r;
      c->k0_mask = &ms;
      c->k0_keep = nullptr;
      r = one ? icikt::host::upload_prepare_pairs(c, X, n_feat, n_samp, flags)
              : icikt::host::upload_and_prepare(c, X, n_feat, n_samp, 0, n_samp, flags);
      c->k0_mask = nullptr;
      if (r) return r;
      c->prepared = true;
      const int64_t n_blocks = one_class ? (int64_t)blocks.size() : n_slices;
      int64_t begin = 0;
      for (int64_t bk = 0; bk < n_blocks; ++bk) {
        int64_t count;
        if (one_class) {
          begin = row_offset(S, blocks[bk].first);
          count = row_offset(S, blocks[bk].second) - begin;
          if (!one) r = icikt_set_pairs_combn(c, S, begin, begin + count);
        } else if (one) {
          count = total;
        } else {
          try { next_slice(cr, &cur, budget, &pi, &pj); } catch (const std::bad_alloc&) {
            return fail(c, ICIKT_E_NOMEM, "class_medians: host allocation failed");
          }
          count = (int64_t)pi.size();
          r = icikt_set_pairs(c, pi.data(), pj.data(), count);
        }
        if (r) return r;
        if (count <= 0 || begin + count > total) return fail(c, ICIKT_E_STATE, "class_medians: the block cut lost its place");
        r = icikt_run_dev(c, perspective, alternative, continuity,
                          run_flags | ((one && c->raw_valid) ? ICIKT_FLAG_REUSE_COUNTS : 0u), c->d_out4.p, nullptr,
                          c->d_reasons.p);
        if (r) return r;
        r = fold(begin, count);
        if (r) return r;
        begin += count;
      }
      if (begin != total) return fail(c, ICIKT_E_STATE, "class_medians: the blocks do not add up to the pair list");
    }
    r = timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_median_select(mc, md.kept.p, c->d_red.p, (int)S, scale_max ? 1 : 0, stage, md.med2.p,
                                          md.n_valid.p, c->stream));
    r = timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    r = icikt::host::download(c, med2, md.med2.p, 2 * (size_t)S * sizeof(double));
    if (!r && n_valid) r = icikt::host::download(c, n_valid, md.n_valid.p, (size_t)S * sizeof(int32_t));
    if (!r) r = icikt::host::download(c, red, c->d_red.p, sizeof(red));
    return r;
  };
  rc = leave(body());
  c->k0_mask = nullptr;
  if (rc) return rc;
  if (reason_counts) for (int r = 0; r < 5; ++r) reason_counts[r] = (int64_t)red[1 + r];
  if (max_taumax && red[0]) {
    const unsigned long long u = (red[0] >> 63) ? (red[0] & 0x7FFFFFFFFFFFFFFFull) : ~red[0];
    std::memcpy(max_taumax, &u, sizeof(double));
  }
  return ICIKT_SUCCESS;
}

}  // namespace

extern "C" {

int icikt_class_medians_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                            const double* global_na, int n_global_na, const int32_t* cls, int n_class, int perspective,
                            int alternative, int continuity, uint32_t flags, int scale_max, double* med2,
                            int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return medians_src(c, MatrixSrc::dense(&v), n_feat, n_samp, global_na, n_global_na, cls, n_class, perspective,
                     alternative, continuity, flags, scale_max, med2, n_valid, max_taumax, reason_counts);
}

int icikt_class_medians_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                           int n_global_na, const int32_t* cls, int n_class, int perspective, int alternative,
                           int continuity, uint32_t flags, int scale_max, double* med2, int32_t* n_valid,
                           double* max_taumax, int64_t* reason_counts) {
  return medians_src(c, MatrixSrc::dense(X), n_feat, n_samp, global_na, n_global_na, cls, n_class, perspective,
                     alternative, continuity, flags, scale_max, med2, n_valid, max_taumax, reason_counts);
}

int icikt_class_medians_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp,
                            const double* global_na, int n_global_na, const int32_t* cls, int n_class, int perspective,
                            int alternative, int continuity, uint32_t flags, int scale_max, double* med2,
                            int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  return medians_src(c, MatrixSrc::csc(X), n_feat, n_samp, global_na, n_global_na, cls, n_class, perspective,
                     alternative, continuity, flags, scale_max, med2, n_valid, max_taumax, reason_counts);
}

}  // extern "C"
