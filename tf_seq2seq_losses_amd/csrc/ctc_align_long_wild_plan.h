// Host-side plan of the tiled best-path alignment with wildcard labels (ctc_align_long_wild.hip, ctc_amd_long_wildcard_best_path):
// the plan of ctc_align_long_plan.h -- the same tile grid, launch schedule and regions at the same offsets -- and behind it three
// per-frame regions.  Plain C++ with no HIP in it, so that tests/tools/long_wild_plan_check.cpp can run it under the host
// sanitizers.  Every byte count is a size_t.
#pragma once
#include <stddef.h>

#include "ctc_align_long_plan.h"

namespace ctc {

struct LongWildPlan {
  LongPlan base;                       // base.total: where the per-frame regions begin
  size_t off_max, off_arg, off_lp, total;
};

// false: what long_plan refuses
inline bool long_wild_plan(int B, int T, int U, int frames_per_tile, LongWildPlan *out) {
  LongWildPlan W;
  if (!long_plan(B, T, U, frames_per_tile, &W.base)) return false;
  const size_t b = (size_t)B, t = (size_t)T;
  size_t o = W.base.total;
  W.off_max = o; o = long_r256(o + b * t * 8);  // m_t, the row maximum: [B][T] float64
  W.off_arg = o; o = long_r256(o + b * t * 4);  // a_t, the lowest token that attains it: [B][T] int32
  W.off_lp = o;  o = long_r256(o + b * t * 8);  // the sweep: LSE_t; the back-trace: lp[t, pi_t]: [B][T] float64
  W.total = o;
  *out = W;
  return true;
}

}  // namespace ctc
