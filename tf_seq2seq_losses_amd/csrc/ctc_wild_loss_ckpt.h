// Host launcher of ctc_wild_loss_ckpt.hip (wildcard CTC gradient from block checkpoints), for that unit and ctc_capi.hip.  Host
// declarations only.
#pragma once
#include "ctc_wild_loss.h"

namespace ctc {

// Frames per checkpoint block, by label positions per lane (NL = 1, 2, 4: U <= 64, 128, 256): F * 64 * NL = 2048 lattice positions
// per block, the most whose alpha rows, emissions and posteriors fit one workgroup's LDS twice over
constexpr int WILD_CKPT_MAX_U = 256;
constexpr int wild_ckpt_frames(int NL) { return 2048 / (64 * NL); }

// U <= 256, with a gradient, each region rounded up to 256 bytes: the chain's float64 state BEFORE every block of F frames
// ([B][ceil(T / F)][S * 64 * NL + 2] doubles, S = 2 classic / 1 simplified), the float32 row statistics ([B][T][4]) and log2 Z ([B]).
// U > 256: wild_loss_workspace_bytes.  Without a gradient: 0
size_t wild_loss_ckpt_workspace_bytes(int kind, int B, int T, int U, bool want_grad);
// grad == nullptr or U > 256: run_wild_loss.  Otherwise two launches: the alpha sweep that stores block checkpoints, the row statistics
// and log2 Z (the loss has the bits of the forward-only call), then the pipelined backward sweep (T == 0: the first alone)
hipError_t run_wild_loss_ckpt(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *ws,
                              hipStream_t st);
// ctc_amd_star_loss_grad_ckpt: the call above with optional wildcards, with the exclusion of the following
// label, or with both, on the same workspace.  grad == nullptr or U > 256: run_wild_loss / run_star_loss with the same flags.
// Neither flag: run_wild_loss_ckpt's kernels.  Otherwise the two launches of the (OPT, XN) kernels, which live in units of their own
// (ctc_wild_loss_ckpt.hip compiled with -DCTC_CKPT_OPT and with -DCTC_STAR) behind the two entry points below it
hipError_t run_star_loss_ckpt(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *ws,
                              hipStream_t st, bool optional_wildcards, bool exclude_next_label);
// (grad != nullptr, U <= 256, a workspace of wild_loss_ckpt_workspace_bytes(want_grad = true))
hipError_t run_wild_loss_ckpt_opt(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *ws,
                                  hipStream_t st);
hipError_t run_wild_loss_ckpt_star(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *ws,
                                   hipStream_t st, bool optional_wildcards);
// ctc_amd_label_posterior_ckpt: `ws` is a workspace of wild_loss_ckpt_workspace_bytes(want_grad = true).  U > 256: run_label_posterior.
// Otherwise two launches: the same alpha sweep, then the backward pipeline whose last stage writes label_posterior [B][T][U],
// blank_posterior [B][T] and, when duration is given, duration / expected_frame [B][U]; no per-frame row and no second read of the matrix
hipError_t run_label_posterior_ckpt(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior, float *blank_posterior,
                                    float *duration, float *expected_frame, char *ws, hipStream_t st);
// ctc_amd_star_label_posterior_ckpt: the call above with optional wildcards, with the exclusion of the
// following label, or with both, on the same workspace.  U > 256: run_label_posterior / run_star_label_posterior with the same
// flags.  Neither flag: run_label_posterior_ckpt.  Otherwise the two launches of the (OPT, XN) kernels, in the two star units
hipError_t run_star_label_posterior_ckpt(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior,
                                         float *blank_posterior, float *duration, float *expected_frame, char *ws, hipStream_t st,
                                         bool optional_wildcards, bool exclude_next_label);
// (U <= 256, a workspace of wild_loss_ckpt_workspace_bytes(want_grad = true))
hipError_t run_label_posterior_ckpt_opt(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior,
                                        float *blank_posterior, float *duration, float *expected_frame, char *ws, hipStream_t st);
hipError_t run_label_posterior_ckpt_star(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior,
                                         float *blank_posterior, float *duration, float *expected_frame, char *ws, hipStream_t st,
                                         bool optional_wildcards);

}  // namespace ctc
