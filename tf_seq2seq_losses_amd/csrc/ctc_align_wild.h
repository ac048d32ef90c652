// Host launcher of ctc_align_wild.hip (forced alignment with wildcard labels), for that unit and ctc_capi.hip.  Host declarations only.
#pragma once
#include "ctc_common.h"

namespace ctc {

constexpr int ALIGN_WILDCARD = -2;  // = CTC_AMD_WILDCARD (include/ctc_amd.h): the label value of a wildcard position
constexpr int ALIGN_OPTIONAL_CLASSIC_MAX_U = 512;  // optional wildcards on the classic lattice: the NL = 16 chain step would spill
constexpr int ALIGN_OPTIONAL = -3;  // = CTC_AMD_OPTIONAL_WILDCARD: a wildcard position that may be skipped (only where
                                    // optional_wildcards is set; a bad label otherwise)

// one workgroup per utterance; the workspace holds, each rounded up to 256 bytes, the back-pointers of ctc_align.hip ([B][T][64]
// words of 1 .. 8 bytes), the float64 log-probability of the path's token on every frame ([B][T]; during the sweep: the frame's
// log-sum-exp) and the int32 argmax token of every frame ([B][T])
size_t align_wild_workspace_bytes(int B, int T, int U);
// frame_window (ctc_amd_windowed_best_path): int32 [B][window_stride >= 2 U] device memory, (first, last) inclusive per label position;
// nullptr runs the kernels of the unwindowed call.  optional_wildcards (ctc_amd_optional_wildcard_best_path): the kernels in which
// ALIGN_OPTIONAL is an optional wildcard, on the same workspace (the back-pointer words have the room); not together with a window
hipError_t run_align_wild(const Problem &p, char *ws, float *score, int *tokens, int *label_index, int *first_frame, int *last_frame,
                          float *label_score, hipStream_t st, const int32_t *frame_window = nullptr, int window_stride = 0,
                          bool optional_wildcards = false);

}  // namespace ctc
