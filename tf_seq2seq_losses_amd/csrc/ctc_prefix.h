// Host launchers of ctc_prefix.hip (CTC prefix scores), for that unit and ctc_capi.hip.  Host declarations only.
#pragma once
#include "ctc_common.h"

namespace ctc {

constexpr int PREFIX_G = 8;  // hypotheses that share one read of the logits in the score kernel (= CTC_AMD_PREFIX_GROUP)
// the row statistics ([B][T] pairs of float32) and one state buffer ([B][N][2 T + 2] float64)
size_t prefix_rows_bytes(int B, int T);
size_t prefix_state_bytes(int B, int T, int N);
hipError_t run_prefix_rows(const Problem &p, void *rows, hipStream_t st);
hipError_t run_prefix_extend(const Problem &p, int N, const void *rows, const double *state_in, const int *last_in, const int *len_in,
                             const int *parent, const int *token, double *state_out, int *last_out, int *len_out, float *full,
                             hipStream_t st);
hipError_t run_prefix_score(const Problem &p, int N, const void *rows, const double *state, const int *last, const int *len,
                            float *score, hipStream_t st);

}  // namespace ctc
