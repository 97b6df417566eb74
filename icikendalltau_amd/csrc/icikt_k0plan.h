// icikt_k0plan.h -- which shape of the pre-pass kernel (icikt_prepass.hip) a launch takes.  Host arithmetic only: no
// device header, so tests/k0plan_print.cpp compiles it with the host compiler alone.  Part of icikt_host.h.
#ifndef ICIKT_K0PLAN_H
#define ICIKT_K0PLAN_H

#include <cstdint>

namespace icikt {
namespace host {

// the shapes, as the debug plan key "k0" numbers them (launch_k0's `shape`)
enum : int {
  K0_SHAPE_LARGE = 0,   // 1 024 threads, one workgroup per CU (k0_prepare_large / large8 by the column length)
  K0_SHAPE_SMALL = 1,   // 256 threads: fits beside a running pair kernel; reached through the plan key only
  K0_SHAPE_PAIR = 2,    // 512 threads x 8 elements, two workgroups per CU: two columns in flight
};

// Column lengths at which the 512-thread shape measured faster than the large one in EVERY repeat of the sweep
// (profiles/k0_two_in_flight.log, section 3: 300 .. 50 000 rows at 512, 1 024 and 2 048 columns on 256 CUs): every
// length from 300 to 10 000 rows at every width, by 8 .. 48 %.  At 12 000 and 12 288 rows it lost at 512 and 1 024
// columns, from 14 000 rows on everywhere (by 12 .. 37 %: the 8 192-element tile of the large shape saves these columns
// tiles and a merge level through the scratch).  Outside the range, and at widths the sweep has no point for (fewer
// than two columns per CU), the large shape stays.
constexpr int K0_PAIR_MIN_ROWS = 300;
constexpr int K0_PAIR_MAX_ROWS = 10000;
constexpr int K0_PAIR_MIN_COLUMNS_PER_CU = 2;

// (rows of a column, columns in the launch, CUs of the device) -> shape.  Two columns in flight on a CU pay when the
// launch has columns to spare; a launch of no more columns than CUs is a single round either way, and there the
// 1 024-thread workgroup is the fastest way through ONE column.
inline int k0_pick_shape(int64_t n, int64_t columns, int cus) {
  if (cus <= 0 || columns <= (int64_t)cus) return K0_SHAPE_LARGE;
  if (columns < (int64_t)K0_PAIR_MIN_COLUMNS_PER_CU * cus) return K0_SHAPE_LARGE;   // (not measured)
  if (n < K0_PAIR_MIN_ROWS || n > K0_PAIR_MAX_ROWS) return K0_SHAPE_LARGE;
  return K0_SHAPE_PAIR;
}

// the same under the debug plan key k0 (-1: the library's choice; 0 | 1 | 2 force a shape)
inline int k0_launch_shape(int k0_override, int64_t n, int64_t columns, int cus) {
  if (k0_override == K0_SHAPE_LARGE || k0_override == K0_SHAPE_SMALL || k0_override == K0_SHAPE_PAIR) return k0_override;
  return k0_pick_shape(n, columns, cus);
}

}  // namespace host
}  // namespace icikt
#endif
