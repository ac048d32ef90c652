// Host launcher of ctc_loss_long.hip (long-form CTC loss and gradient with wildcard labels: the sum-product lattice of
// ctc_wild_loss.hip on the tiles of ctc_align_long.hip), for that unit and ctc_capi.hip.  Host declarations only; the plan is
// ctc_loss_long_plan.h.
#pragma once
#include "ctc_common.h"
#include "ctc_loss_long_plan.h"

namespace ctc {

constexpr int LONG_LOSS_WILDCARD = -2;  // = CTC_AMD_WILDCARD (include/ctc_amd.h): the label value of a wildcard position
constexpr int LONG_LOSS_OPTIONAL = -3;  // = CTC_AMD_OPTIONAL_WILDCARD: ... that may take no frame (optional_wildcards alone)

// grad == nullptr (a plan with want_grad == 0 suffices): P.launches alpha tile launches and the finish kernel.  Otherwise (want_grad
// == 1) the same, bit for bit, then P.launches beta tile launches and the row stage.  T == 0: the finish kernel alone.  `ws` holds
// P.total bytes and may hold anything.  A plan of long_loss_ckpt_plan with a gradient (P.ckpt; grad != nullptr) runs the
// checkpointed schedule instead: the alpha tiles that keep a checkpoint per tile and the finish kernel, then per reverse
// anti-diagonal the alpha tiles again, the beta tiles and, for d < P.J, the row stage of time block d.  The same bits.
// frame_window: nullptr, or [B][window_stride >= 2 U] int32 pairs (first, last), the frames position i may own (DESIGN.md section
// 5.25); it selects the WIN instantiations of the alpha and beta tiles and changes nothing else.
// optional_wildcards (ctc_amd_long_optional_wildcard_*): the OPT instantiations, on a plan made with opt = 1
// (the two further column buffers) and without a window.
hipError_t run_loss_long(const Problem &p, const LongLossPlan &P, float wildcard_log_weight, const float *d_loss, float *loss, void *grad,
                         char *ws, hipStream_t st, const int32_t *frame_window = nullptr, int window_stride = 0,
                         bool optional_wildcards = false);

// ctc_amd_long_label_posterior: the checkpointed schedule above (P.L) with the posterior stage in the row stage's place.  Per time
// block d < P.L.J one launch writes label_posterior (nullptr: not wanted) and blank_posterior of the block's frames and carries the
// per-position sums and the peak in the workspace; the stage of block 0 writes duration / expected_frame and peak_posterior /
// peak_frame (each pair both or neither).  T == 0: the finish kernel and, for the [B][U] outputs, one launch.  `ws` holds P.total
// bytes and may hold anything.  frame_window: as above.
hipError_t run_long_label_posterior(const Problem &p, const LongPostPlan &P, float wildcard_log_weight, float *loss, float *label_posterior,
                                    float *blank_posterior, float *duration, float *expected_frame, float *peak_posterior,
                                    int *peak_frame, char *ws, hipStream_t st, const int32_t *frame_window = nullptr,
                                    int window_stride = 0, bool optional_wildcards = false);

}  // namespace ctc
