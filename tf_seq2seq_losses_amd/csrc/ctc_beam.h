// Host launcher of ctc_beam.hip (prefix beam search), for that unit and ctc_capi.hip.  Host declarations only.
#pragma once
#include "ctc_common.h"

namespace ctc {

// the effective token cut min(top_k, V - 1); workspace: the row-stage records ([B][T][4 + 2 K] words) plus the prefix trie
// ([B][1 + beam_width * T] nodes of 8 bytes), each rounded up to 256 bytes
int beam_effective_k(int V, int top_k);
size_t beam_workspace_bytes(int B, int T, int V, int beam_width, int top_k);
hipError_t run_beam(const Problem &p, int beam_width, int top_k, int nbest, char *ws, float *score, int *decoded, int *decoded_length,
                    hipStream_t st);

}  // namespace ctc
