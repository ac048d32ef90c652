// Host launcher of ctc_align_long_star.hip (long-form forced alignment with optional wildcards and the exclusion of the next label),
// for that unit and ctc_capi.hip.  Host declarations only; the plan is ctc_align_long_star_plan.h.
#pragma once
#include "ctc_align_long_star_plan.h"
#include "ctc_common.h"

namespace ctc {

// P.base.launches tile launches (one anti-diagonal each), one trace workgroup per utterance, one frame-parallel launch when
// first_frame or last_frame is given and one more when label_score is; `ws` holds P.total bytes of the plan made for p.kind.  At
// least one of the two keywords is set: the call with neither is run_align_long_wild's
hipError_t run_align_long_star(const Problem &p, const LongStarPlan &P, char *ws, float *score, int *tokens, int *label_index,
                               int *first_frame, int *last_frame, float *label_score, hipStream_t st, bool optional_wildcards,
                               bool exclude_next_label);

}  // namespace ctc
