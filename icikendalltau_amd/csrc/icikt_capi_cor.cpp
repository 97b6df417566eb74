// icikt_capi_cor.cpp -- the C-ABI entry of cor_fast (icikt_cor_pairs_f64): Pearson and Spearman cor.test for column
// pairs, sequencing the kernels of icikt_cor.hip on a context's stream.  The context, the entry checks and the
// timers it shares with the pair engine are in icikt_capi.cpp (declared in icikt_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::check_pair_list;
using icikt::host::check_shape;
using icikt::host::fail;
using icikt::host::timer_begin;
using icikt::host::timer_end;
using icikt::host::use_device;

// Spearman's exact null distribution for n = 2 .. 9 (prho, AS 89 as R enumerates it): for each n, upper[k] = the
// permutations whose S = sum (i - perm(i))^2 is >= 2 k, k = 0 .. (n^3 - n) / 6 (S is always even)
static std::vector<uint32_t> cor_prho_table() {
  std::vector<uint32_t> out;
  for (int n = 2; n <= 9; ++n) {
    const int kmax = (n * n * n - n) / 6;
    std::vector<uint32_t> cnt((size_t)kmax + 1, 0u);
    int perm[9];
    for (int i = 0; i < n; ++i) perm[i] = i;
    do {
      int sq = 0;
      for (int i = 0; i < n; ++i) sq += (i - perm[i]) * (i - perm[i]);
      cnt[(size_t)(sq / 2)] += 1;
    } while (std::next_permutation(perm, perm + n));
    std::vector<uint32_t> up((size_t)kmax + 1);
    uint32_t acc = 0;
    for (int k = kmax; k >= 0; --k) { acc += cnt[(size_t)k]; up[(size_t)k] = acc; }
    out.insert(out.end(), up.begin(), up.end());
  }
  return out;
}

extern "C" {

// cor_fast: pre-pass (K_PREPARE timer), pair products (K_PAIRS), cor.test epilogue (K_EPILOGUE), all on c->stream.
//   Pearson, no NA             Z^T Z of the mean-shifted, power-of-two-scaled columns, less Σz_i Σz_j / n: 64 x 64
//                              tiles when the list is all of combn(S, 2) (then the self pairs, or not), one wave per
//                              pair otherwise
//   Pearson, pairwise          one wave per pair, two passes over the raw columns: the jointly present rows' mean and
//                              spread, then their centred, scaled and corrected sums (numerics)
//   Spearman, no NA            as Pearson, on the centred doubled ranks (integers: the sums are exact)
//   Spearman, pairwise         one workgroup per pair: the subset ranks from prefix counts, sums in int64
int icikt_cor_pairs_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                        const int32_t* pi, const int32_t* pj, int64_t n_pairs, int method, int pairwise,
                        int alternative, int continuity, uint32_t flags, double* out3, int32_t* reasons) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return icikt_cor_pairs_in(c, &v, n_feat, n_samp, pi, pj, n_pairs, method, pairwise, alternative, continuity, flags, out3,
                            reasons);
}

int icikt_cor_pairs_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const int32_t* pi,
                       const int32_t* pj, int64_t n_pairs, int method, int pairwise, int alternative, int continuity,
                       uint32_t flags, double* out3, int32_t* reasons) {
  if (!c) return ICIKT_E_INVALID;
  int rc = icikt::host::check_view(c, "cor", X, n_feat, n_samp);
  if (rc) return rc;
  rc = check_pair_list(c, "cor", pi, pj, n_pairs, n_samp);
  if (rc) return rc;
  if (method != ICIKT_METHOD_PEARSON && method != ICIKT_METHOD_SPEARMAN)
    return fail(c, ICIKT_E_INVALID, "cor: method must be pearson (0) or spearman (1)");
  if (alternative < ICIKT_ALT_TWO_SIDED || alternative > ICIKT_ALT_GREATER)
    return fail(c, ICIKT_E_INVALID, "cor: alternative must be two.sided (0), less (1) or greater (2)");
  if (n_pairs == 0) return ICIKT_SUCCESS;
  if (!out3 || !reasons) return fail(c, ICIKT_E_INVALID, "cor: null output");
  rc = use_device(c);
  if (rc) return rc;
  rc = icikt_set_pairs(c, pi, pj, n_pairs);
  if (rc) return rc;
  // the list is all of combn(S, 2) (optionally followed by the S self pairs, as setup_comparisons(diag_good = FALSE)
  // makes it): one tile kernel covers it
  const int64_t ncombn = n_samp * (n_samp - 1) / 2;
  int full = 0;   // 1: combn, 2: combn + self pairs
  if (n_pairs == ncombn || n_pairs == ncombn + n_samp) {
    full = n_pairs == ncombn ? 1 : 2;
    int64_t p = 0;
    for (int64_t i = 0; i < n_samp && full; ++i)
      for (int64_t j = i + 1; j < n_samp; ++j, ++p)
        if (pi[p] != i || pj[p] != j) { full = 0; break; }
    for (int64_t i = 0; full == 2 && i < n_samp; ++i)
      if (pi[ncombn + i] != i || pj[ncombn + i] != i) full = 0;
  }
  const icikt::host::PinnedScope scope(c, flags);
  icikt_ctx::CorBufs& cb = c->cor;
  auto body = [&]() -> int {
    if (!cb.prho_ready) {
      const std::vector<uint32_t> t = cor_prho_table();
      HIPCHK(c, cb.prho.reserve(t.size()));
      int r = icikt::host::upload_sync(c, cb.prho.p, t.data(), t.size() * sizeof(uint32_t));
      if (r) return r;
      cb.prho_ready = true;
    }
    if (n_feat > 0) {
      int r = icikt::host::upload_and_prepare(c, *X, n_feat, n_samp, 0, n_samp, 0u, false, nullptr,
                                              icikt::host::kPrepassNone);
      if (r) return r;
    }
    const int64_t n = n_feat;
    const bool spearman = method == ICIKT_METHOD_SPEARMAN;
    // (dense Spearman sums of centred doubled ranks are integers below (n^3 - n) / 3 < 2^53 for every n the library
    // takes: exact in f64; the pairwise kernel sums in int64)
    const bool spearman_pw = spearman && pairwise;
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    const int prep_blocks = (int)std::max<int64_t>(1, std::min<int64_t>({n_samp, 2048,
        std::max<int64_t>(1, ((int64_t)1 << 29) / ((int64_t)np2 * 12))}));
    const int pw_blocks = (int)std::max<int64_t>(1, std::min<int64_t>({n_pairs, 4096,
        std::max<int64_t>(1, ((int64_t)1 << 29) / ((2 * n + 1) * 4))}));
    const size_t nS = (size_t)std::max<int64_t>(n * n_samp, 1);
    HIPCHK(c, cb.z.reserve(nS));
    HIPCHK(c, cb.colss.reserve((size_t)std::max<int64_t>(n_samp, 1)));
    HIPCHK(c, cb.colsum.reserve((size_t)std::max<int64_t>(n_samp, 1)));
    HIPCHK(c, cb.cnt.reserve((size_t)std::max<int64_t>(n_samp, 1)));
    HIPCHK(c, cb.flags.reserve((size_t)std::max<int64_t>(n_samp, 1)));
    HIPCHK(c, cb.acc.reserve((size_t)n_pairs));
    HIPCHK(c, c->d_out4.reserve((size_t)n_pairs * 3));
    HIPCHK(c, c->d_reasons.reserve((size_t)n_pairs));
    icikt::CorPrep cp{};
    cp.X = c->d_X.p;
    cp.ld = n;
    cp.n = n;
    cp.S = (int)n_samp;
    cp.method = method;
    cp.Z = cb.z.p;
    cp.cnt = cb.cnt.p;
    cp.colss = cb.colss.p;
    cp.colsum = cb.colsum.p;
    cp.flags = cb.flags.p;
    cp.np2 = np2;
    if (spearman) {
      HIPCHK(c, cb.order.reserve(3 * nS));
      HIPCHK(c, cb.keys.reserve((size_t)prep_blocks * np2));
      HIPCHK(c, cb.scratch.reserve(std::max<size_t>((size_t)prep_blocks * np2,
                                                    spearman_pw ? (size_t)pw_blocks * (size_t)(2 * n + 1) : 0)));
      cp.ord = cb.order.p;
      cp.gs = cb.order.p + nS;
      cp.ge = cb.order.p + 2 * nS;
      cp.keys = reinterpret_cast<uint64_t*>(cb.keys.p);
      cp.idx = cb.scratch.p;
    }
    int r = timer_begin(c, ICIKT_K_PREPARE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_cor_prep(cp, prep_blocks, c->stream));
    r = timer_end(c, ICIKT_K_PREPARE, flags);
    if (!r) r = timer_begin(c, ICIKT_K_PAIRS, flags);
    if (r) return r;
    if (spearman_pw) {
      HIPCHK(c, icikt::launch_cor_spearman_pw(cp, c->d_pi.p, c->d_pj.p, n_pairs, pw_blocks, cb.scratch.p, cb.acc.p,
                                              c->stream));
    } else if (full && !pairwise) {
      HIPCHK(c, icikt::launch_cor_tile(cp, full == 2, cb.acc.p, c->stream));
    } else {
      HIPCHK(c, icikt::launch_cor_dots(cp, pairwise, c->d_pi.p, c->d_pj.p, n_pairs, cb.acc.p, c->stream));
    }
    r = timer_end(c, ICIKT_K_PAIRS, flags);
    if (!r) r = timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_cor_epilogue(cb.acc.p, n_pairs, method, pairwise, alternative, continuity, cb.prho.p,
                                         c->d_out4.p, c->d_reasons.p, c->stream));
    r = timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (!r) r = icikt::host::download(c, out3, c->d_out4.p, (size_t)n_pairs * 3 * sizeof(double));
    if (!r) r = icikt::host::download(c, reasons, c->d_reasons.p, (size_t)n_pairs * sizeof(int32_t));
    return r;
  };
  return icikt::host::end_call(c, "cor", body());
}

}  // extern "C"
