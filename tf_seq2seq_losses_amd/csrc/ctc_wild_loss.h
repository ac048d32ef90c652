// Host launcher of ctc_wild_loss.hip (CTC loss and gradient with wildcard labels), for that unit and ctc_capi.hip.  Host declarations only.
#pragma once
#include "ctc_common.h"

namespace ctc {

constexpr int WILD_LOSS_WILDCARD = -2;  // = CTC_AMD_WILDCARD (include/ctc_amd.h): the label value of a wildcard position
constexpr int WILD_LOSS_OPTIONAL = -3;  // = CTC_AMD_OPTIONAL_WILDCARD: a wildcard position that may also take no frame (only where
                                        // optional_wildcards is set; a bad label otherwise)

// forward only: no workspace.  With a gradient, each rounded up to 256 bytes: the chain's float64 state of every frame ([B][T][S * 64 *
// NL + 2] doubles, S = 2 classic / 1 simplified; overwritten by the posteriors), the float32 row statistics ([B][T][4]) and log2 Z ([B])
size_t wild_loss_workspace_bytes(int kind, int B, int T, int U, bool want_grad);
// grad == nullptr: one launch, the loss alone.  Otherwise the alpha sweep, the beta sweep and the row stage (T == 0: the first alone).
// frame_window (ctc_amd_windowed_loss_grad / _label_posterior): int32 [B][window_stride >= 2 U] device memory, (first, last) inclusive
// per label position; nullptr runs the kernels of the unwindowed call.  optional_wildcards (ctc_amd_optional_wildcard_loss_grad /
// _label_posterior): the kernels in which WILD_LOSS_OPTIONAL is an optional wildcard; not together with a window
hipError_t run_wild_loss(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *ws, hipStream_t st,
                         const int32_t *frame_window = nullptr, int window_stride = 0, bool optional_wildcards = false);
// ctc_amd_label_posterior: the alpha sweep of the gradient path (so `ws` is a workspace of wild_loss_workspace_bytes(want_grad = true)),
// the beta sweep that writes label_posterior [B][T][U] and blank_posterior [B][T] (none when T == 0) and, when duration is given,
// one launch for duration / expected_frame [B][U] (none when U == 0)
hipError_t run_label_posterior(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior, float *blank_posterior,
                               float *duration, float *expected_frame, char *ws, hipStream_t st, const int32_t *frame_window = nullptr,
                               int window_stride = 0, bool optional_wildcards = false);

}  // namespace ctc
