// Host launcher of ctc_align_long.hip (long-form forced alignment, the lattice tiled over label blocks x time blocks), for that unit
// and ctc_capi.hip.  Host declarations only; the plan (tile grid, launch schedule, workspace offsets) is ctc_align_long_plan.h.
#pragma once
#include "ctc_align_long_plan.h"
#include "ctc_common.h"

namespace ctc {

// P.launches tile launches (one anti-diagonal each, B x tiles-on-the-diagonal workgroups), one trace workgroup per utterance and,
// when first_frame or last_frame is given, one frame-parallel launch; `ws` holds P.total bytes
hipError_t run_align_long(const Problem &p, const LongPlan &P, char *ws, float *score, int *tokens, int *label_index, int *first_frame,
                          int *last_frame, hipStream_t st);

}  // namespace ctc
