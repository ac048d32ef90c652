// Host launcher of ctc_align_long_wild.hip (long-form forced alignment with wildcard labels: the tiled lattice of
// ctc_align_long.hip with the wildcard positions and per-label scores of ctc_align_wild.hip), for that unit and ctc_capi.hip.
// Host declarations only; the plan is ctc_align_long_wild_plan.h.
#pragma once
#include "ctc_align_long_wild_plan.h"
#include "ctc_common.h"

namespace ctc {

// P.base.launches tile launches (one anti-diagonal each), one trace workgroup per utterance, one frame-parallel launch when
// first_frame or last_frame is given and one more when label_score is; `ws` holds P.total bytes
hipError_t run_align_long_wild(const Problem &p, const LongWildPlan &P, char *ws, float *score, int *tokens, int *label_index,
                               int *first_frame, int *last_frame, float *label_score, hipStream_t st,
                               const int32_t *frame_window = nullptr, int window_stride = 0);  // (as run_align_wild's; frames are absolute)

}  // namespace ctc
