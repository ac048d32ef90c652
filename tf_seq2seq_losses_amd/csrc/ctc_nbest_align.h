// Host launcher of ctc_nbest_align.hip (N-best forced alignment), for that unit and ctc_capi.hip.  Host declarations only.
#pragma once
#include "ctc_common.h"

namespace ctc {

// one workgroup per utterance and group of NBEST_G hypotheses (ctc_launch.h); the workspace holds the back-pointers alone
// ([B * N][T][64] words of 1 .. 8 bytes, the word of ctc_align.hip), rounded up to 256 bytes
size_t nbest_align_workspace_bytes(int B, int T, int U, int N);
hipError_t run_nbest_align(const Problem &p, int N, char *ws, float *score, int *tokens, int *label_index, int *first_frame,
                           int *last_frame, hipStream_t st);

}  // namespace ctc
