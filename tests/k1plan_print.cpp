// k1plan_print.cpp -- prints what csrc/icikt_k1plan.h decides, one JSON value per line, for tests/test_k1plan_host.py.
// Host code only: no device header, no library.  One case per line of standard input:
//   plan N NPAIRS NCU TIED NTG_HINT GROUP_HINT KEY=VALUE|-    the pair kernel's launch plan, Wp as the library derives it
//                                                            from N; one plan key (np half hyb tgmax list solo split
//                                                            waves wpb) or none -> the fields of K1Plan
//   tied LONG N M  then M x (ntg tfill e0 e1 ngroups nna)     the verdict on M columns' statistics
//                                                            -> [tied_state, ntg_hint, group_hint]
//   combn S BEGIN END                                        the pairs of a combn range -> [[pi ...], [pj ...]]
//   units NP P pi[P] pj[P]                                   the task list -> [p0, p1, p0, p1, ...]
//   chunkunits S NP K end[K]                                 the full triangle's tasks by the chunk of their last column, from
//                                                            combn_chunk_units called chunk after chunk (columns
//                                                            [end[q-1], end[q]) arrive with chunk q) -> [first[K+1], units]
//   chunkorder NP P pi[P] pj[P] K end[K]                     the same shape from build_units followed by order_units_by_chunk
//   grid NP HALF_ITEMS WPB SPLIT OPTS COUNT PER_CU NCU GRIDMULT GRIDCAP
//                                                            the grid of a launch -> [split, opts, blocks, persistent]
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "icikt_k1plan.h"

namespace kp = icikt::host;

static void print_ints(const std::vector<int32_t>& v) {
  std::printf("[");
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", (int)v[i]);
  std::printf("]");
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "plan") {
      long long n_pairs;
      int n, n_cu, tied, ntg, group;
      std::string kv;
      if (!(std::cin >> n >> n_pairs >> n_cu >> tied >> ntg >> group >> kv)) return 2;
      kp::PlanOverride ov;
      if (kv != "-") {
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) return 2;
        const std::string key = kv.substr(0, eq);
        const int val = std::atoi(kv.c_str() + eq + 1);
        if (key == "np") ov.np = val;
        else if (key == "half") ov.half = val;
        else if (key == "hyb") ov.hyb = val;
        else if (key == "tgmax") { ov.has_tgmax = true; ov.tgmax = val; }
        else if (key == "list") ov.list = val;
        else if (key == "solo") ov.solo = val;
        else if (key == "split") ov.split = val;
        else if (key == "waves") ov.waves = val;
        else if (key == "wpb") ov.wpb = val;
        else return 2;
      }
      const int Wp = (n + 63) / 64 + 1;   // (prepare_alloc: W + 1, one zero guard word)
      const kp::K1Plan pl = kp::plan_k1(n, Wp, n_pairs, n_cu, ov, tied != 0, ntg, group);
      std::printf("[%d, %d, %zu, %d, %d, %d, %d, %d]\n", pl.np, pl.wpb, pl.lds_bytes, pl.perpair_bytes, pl.opts, pl.half_items,
                  pl.stride, pl.split);
    } else if (cmd == "tied") {
      int long_cols, n, m;
      if (!(std::cin >> long_cols >> n >> m) || m < 0) return 2;
      std::vector<icikt::ColStats> st((size_t)m);
      for (auto& t : st) {
        t = icikt::ColStats{};
        if (!(std::cin >> t.ntg >> t.tfill >> t.e0 >> t.e1 >> t.ngroups >> t.nna)) return 2;
      }
      const kp::TieVerdict v = kp::tie_verdict(st, n, long_cols != 0);
      std::printf("[%d, %d, %d]\n", v.tied_state, v.ntg_hint, v.group_hint);
    } else if (cmd == "combn") {
      long long S, begin, end;
      if (!(std::cin >> S >> begin >> end)) return 2;
      std::vector<int32_t> pi, pj;
      kp::combn_pairs(S, begin, end, pi, pj);
      std::printf("[");
      print_ints(pi);
      std::printf(", ");
      print_ints(pj);
      std::printf("]\n");
    } else if (cmd == "units") {
      int np;
      long long P;
      if (!(std::cin >> np >> P) || P < 0) return 2;
      std::vector<int32_t> pi((size_t)P), pj((size_t)P), u;
      for (auto& x : pi) if (!(std::cin >> x)) return 2;
      for (auto& x : pj) if (!(std::cin >> x)) return 2;
      kp::build_units(pi, pj, P, np, u);
      print_ints(u);
      std::printf("\n");
    } else if (cmd == "chunkunits" || cmd == "chunkorder") {
      std::vector<int32_t> u;
      std::vector<int> first;
      std::vector<int64_t> ends;
      auto read_ends = [&ends]() {
        long long K;
        if (!(std::cin >> K) || K < 0) return false;
        ends.resize((size_t)K);
        for (auto& e : ends) if (!(std::cin >> e)) return false;
        return true;
      };
      if (cmd == "chunkunits") {
        long long S;
        int np;
        if (!(std::cin >> S >> np) || S < 0 || !read_ends()) return 2;
        u.resize((size_t)(S * (S - 1) / 2 + S + 8) * 2);   // (the staging buffer's capacity: upload_prepare_pairs)
        first.assign(1, 0);
        int64_t cb = 0;
        for (const int64_t ce : ends) {
          first.push_back(first.back() + (int)kp::combn_chunk_units(S, cb, ce, np, u.data() + 2 * (size_t)first.back()));
          cb = ce;
        }
        u.resize(2 * (size_t)first.back());
      } else {
        int np;
        long long P;
        if (!(std::cin >> np >> P) || P < 0) return 2;
        std::vector<int32_t> pi((size_t)P), pj((size_t)P);
        for (auto& x : pi) if (!(std::cin >> x)) return 2;
        for (auto& x : pj) if (!(std::cin >> x)) return 2;
        if (!read_ends()) return 2;
        kp::build_units(pi, pj, P, np, u);
        kp::order_units_by_chunk(u, pi.data(), pj.data(), ends, first);
      }
      std::printf("[");
      print_ints(std::vector<int32_t>(first.begin(), first.end()));
      std::printf(", ");
      print_ints(u);
      std::printf("]\n");
    } else if (cmd == "grid") {
      kp::K1Plan pl{};
      int count, per_cu, n_cu, mult, cap;
      if (!(std::cin >> pl.np >> pl.half_items >> pl.wpb >> pl.split >> pl.opts >> count >> per_cu >> n_cu >> mult >> cap)) return 2;
      const kp::K1Grid g = kp::k1_grid(pl, count, per_cu, n_cu, mult, cap);
      std::printf("[%d, %d, %d, %d]\n", g.split, g.opts, g.blocks, g.persistent ? 1 : 0);
    } else {
      return 2;
    }
  }
  return 0;
}
