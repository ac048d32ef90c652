/*
 * ctc_amd.h -- C ABI of the MI355X-native CTC loss (loss, analytic gradient, analytic Hessian).
 *
 * This is the drop-in boundary for the hot path of alexeytochin/tf_seq2seq_losses.  The reference has
 * no FFI of its own (it is pure Python on TensorFlow); the entry points below are what a binding for
 * its two public functions and its loss-data properties would call.  Each one cites the reference
 * interface it replaces (paths relative to the reference repo, v0.3.0).
 *
 * Conventions
 *   - All pointers are DEVICE pointers (HIP, gfx950) unless a parameter says "host".
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Every entry point is
 *     asynchronous on that stream, performs no allocation, no host<->device copy and no device
 *     synchronisation, and is therefore capturable into a hipGraph.
 *   - The caller owns every buffer, including the workspace (size from ctc_amd_workspace_bytes).
 *     Outputs are fully overwritten.  The library keeps no global state besides a thread-local
 *     error string and the test-only tier override of ctc_amd_debug_override (never set by the product path);
 *     calls are re-entrant for distinct (stream, workspace) pairs.  The override is a plain process-wide
 *     variable: ctc_amd_debug_override is NOT thread-safe against calls running in other threads -- set it
 *     between calls, from the one thread that makes them (tests and benchmarks only).
 *   - Layouts are dense row-major: logits[B][T][V] float32, labels[B][label_stride] int32,
 *     label_length[B], logit_length[B] int32, loss[B], grad[B][T][V], hess[B][T][V][T][V] float32.
 *   - `U` is a static upper bound on label_length (the reference uses the dynamic max(label_length),
 *     base_loss.py:482-486; any U >= max(label_length) gives identical loss/gradient/Hessian because
 *     the extra lattice states stay at log 0).  A sample with label_length[b] > U gets loss = +inf.
 *   - What the kernels make of out-of-range lengths and labels (logit_length outside [0, T], negative label_length,
 *     label_length > U, label positions beyond label_stride, labels outside [0, V) or equal to the blank) is ONE contract for
 *     every entry point: DESIGN.md section 5.8; its code is csrc/ctc_common.h behind struct Problem.
 *   - Frames at or beyond logit_length[b], label positions at or beyond label_length[b] and the elements between V and the row
 *     stride are never interpreted (they may hold NaN or anything else), and the workspace and the outputs may hold anything on
 *     entry: none of it changes a bit of any result ("Ownership").
 *   - Return value: 0 on success, negative CTC_AMD_E* code otherwise; ctc_amd_last_error() has text.
 *     Not errors (reference semantics, classic_ctc_loss.py:50-52, base_loss.py:240-245,283-288):
 *     infeasible alignment => loss = +inf, gradient = 0, Hessian = 0; B == 0; T == 0.
 */
#ifndef CTC_AMD_H
#define CTC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTC_AMD_ABI_VERSION 6

/* lattice variant */
#define CTC_AMD_CLASSIC 0    /* classic_ctc_loss.py:33-70   (collapse repeats, then drop blanks)   */
#define CTC_AMD_SIMPLIFIED 1 /* simplified_ctc_loss.py:32-67 (drop blanks only)                     */

/* what the float input is / what the derivatives are taken with respect to */
#define CTC_AMD_WRT_LOGITS 0   /* input = logits; log_softmax fused (base_loss.py:59, tools.py:27-40);
                                  derivatives w.r.t. logits (what tf.GradientTape returns to the user) */
#define CTC_AMD_WRT_LOGPROBS 1 /* input = log-probabilities treated as independent variables
                                  (base_loss.py:71-99); derivatives w.r.t. them (loss_data.gradient /
                                  loss_data.hessian, base_loss.py:186-268)                            */

/* error codes */
#define CTC_AMD_OK 0
#define CTC_AMD_EINVAL (-1)     /* bad argument (null pointer, negative size, unsupported shape)      */
#define CTC_AMD_EWORKSPACE (-2) /* workspace too small                                                */
#define CTC_AMD_EHIP (-3)       /* HIP runtime error (launch failure)                                 */
#define CTC_AMD_ELABEL (-4)     /* ctc_amd_check_labels: a label outside [0, V) or equal to the blank */

/* Limits (CTC_AMD_EINVAL beyond them; the reference has none, its cost just grows):
 *   U <= CTC_AMD_MAX_U          label positions (16 per lane of one wavefront)
 *   V <= CTC_AMD_MAX_V          tokens for loss / gradient / alpha-beta (one 64 KB LDS token row per wavefront)
 *   V <= CTC_AMD_MAX_V_HESSIAN  tokens for ctc_amd_hessian / ctc_amd_hvp (V + 4 floats of LDS per wavefront)
 * ctc_amd_best_path takes V <= CTC_AMD_MAX_V as well (it stages no row in LDS; the limit is the ABI's, kept uniform).
 * ctc_amd_long_best_path, ctc_amd_long_wildcard_best_path and ctc_amd_long_wildcard_loss_grad alone take U <= CTC_AMD_LONG_MAX_U
 * (they spread the label axis over workgroups, 1024 positions each).
 * ctc_amd_loss_grad* / ctc_amd_grad_resume / ctc_amd_alpha_beta: vector (16-byte / 8-byte) row accesses are used when V, the
 * strides AND the base pointers are aligned; any other alignment runs element-wise paths with identical results.
 * ctc_amd_hessian / ctc_amd_hvp require 16-byte aligned tensor pointers (CTC_AMD_EINVAL otherwise). */
#define CTC_AMD_MAX_U 1024
#define CTC_AMD_MAX_V 16384
#define CTC_AMD_MAX_V_HESSIAN 16380

/* selector for ctc_amd_workspace_bytes */
#define CTC_AMD_WS_LOSS_GRAD 0
#define CTC_AMD_WS_ALPHA_BETA 1
#define CTC_AMD_WS_HESSIAN 2
#define CTC_AMD_WS_HVP 3
/* ctc_amd_loss_grad* / ctc_amd_grad_resume with wrt == CTC_AMD_WRT_LOGITS and float32 (or 8-byte aligned bfloat16) tensors:
 * the workspace of the pipeline such a call selects -- checkpoint rows only when that is a fused tier (64 MB instead of
 * 680 MB at B=256 T=1000 U=128).  CTC_AMD_WS_LOSS_GRAD stays valid for every call (log-probability input, any format). */
#define CTC_AMD_WS_LOSS_GRAD_LOGITS 4

/* element types of the producer formats (ctc_amd_loss_grad_ex) */
#define CTC_AMD_F32 0
#define CTC_AMD_BF16 1
#define CTC_AMD_F16 2 /* IEEE half: read / written by the three-kernel pipeline (the fused tiers take float32 and bfloat16) */

/* ABI version of the loaded library (== CTC_AMD_ABI_VERSION of the header it was built from). */
int ctc_amd_abi_version(void);

/* Thread-local text of the last error returned on this thread ("" if none). */
const char *ctc_amd_last_error(void);

/* Name of the kernel pipeline ctc_amd_loss_grad would run for contiguous float32 tensors of these shapes ("fused6",
 * "fused5" or "v1"); diagnostic only (benchmarks and tests report it), never needed for correctness. */
const char *ctc_amd_pipeline_name(int kind, int wrt, int B, int T, int V, int U, int want_grad);

/*
 * Diagnostic override, for parity tests and benchmarks only (process-wide; set it between calls, not during one):
 *   key "pipeline": "" (best eligible tier, default), "v1", "fused5" -- forces a lower tier of ctc_amd_loss_grad
 *   key "hessian":  "" (default) or "slab" -- the general Hessian kernel also for labels of <= 32 positions
 *   key "hvp":      "" (default) or "v1"   -- the log-domain Hessian-vector pipeline also where the fused kernel applies
 * The library never reads the environment.  Returns CTC_AMD_EINVAL for an unknown key or value.
 */
int ctc_amd_debug_override(const char *key /*host*/, const char *value /*host*/);

/*
 * Diagnostic (tests/tools/soak.py, the parity tests): byte offset, inside the workspace of a float32 logits call of these
 * shapes (CTC_AMD_WS_LOSS_GRAD_LOGITS layout), of the int32[B] flag words the linear-domain fused kernel leaves -- 0 = the
 * utterance was computed in the linear domain, != 0 = it was redone by the log-domain roles (bits D1..D7).
 * Returns CTC_AMD_EINVAL when that call would not run the "fused6" pipeline.
 */
int ctc_amd_debug_flags_offset(int kind, int B, int T, int V, int U, size_t *out_offset /*host*/);
/* The same for the fused Hessian-vector kernel: offset of its int32[B] flag words inside a CTC_AMD_WS_HVP workspace
 * (CTC_AMD_EINVAL for shapes ctc_amd_hvp does not run that kernel for). */
int ctc_amd_debug_hvp_flags_offset(int kind, int B, int T, int V, int U, size_t *out_offset /*host*/);

/*
 * out2[0] = sum of the finite entries of loss[B], out2[1] = their number (as float): the two scalars a data-parallel
 * training loop all-reduces (tf.reduce_sum / reduce_mean of the loss: README.md:62, tests/benchmark.py:199), in one launch.
 * Asynchronous on `stream` like the compute entry points.
 */
int ctc_amd_reduce_loss(const float *loss, int B, float *out2, void *stream);

/*
 * Opt-in validation of the labels (the ONLY entry point that synchronises the stream and allocates -- a few bytes from the
 * stream-ordered pool; keep it off the hot path).  Returns CTC_AMD_ELABEL if any label inside label_length (and inside
 * label_stride) lies outside [0, V) or equals blank_index; a row with label_length > U is infeasible as a whole (DESIGN.md
 * section 5.8) and none of its labels is looked at.  Without this check such a label is not an error in the
 * compute entry points: it is an impossible emission, the sample comes out infeasible (loss +inf, zero gradient).
 * Replaces: the InvalidArgumentError of tf.gather on TF-CPU for out-of-range labels (base_loss.py:328-344).
 */
int ctc_amd_check_labels(const int32_t *labels, int label_stride, const int32_t *label_length, int blank_index,
                         int B, int V, int U, void *stream);

/*
 * Measurement aid (bench.py's box probe): copies `bytes` (a multiple of 16) from src to dst with the access shape of the
 * kernels' row traffic (16 bytes per lane, non-temporal stores), asynchronously on `stream`.  Not part of the hot path.
 */
int ctc_amd_probe_copy(void *dst, const void *src, size_t bytes, void *stream);

/*
 * Measurement aid (bench.py --emulate-collective): ONE workgroup of `threads` threads holding `lds_bytes` of LDS that polls
 * the device clock for `microseconds` and exits -- the footprint of a latency-bound RCCL all-reduce kernel, to measure on
 * one GPU whether such a kernel runs beside the loss kernel or waits for its tail.  Asynchronous on `stream`.
 */
int ctc_amd_probe_spin(int threads, int lds_bytes, float microseconds, void *stream);

/* Bytes of device workspace the call selected by `what` needs for these shapes. */
int ctc_amd_workspace_bytes(int what, int kind, int B, int T, int V, int U, size_t *out_bytes /*host*/);

/*
 * Loss and (optionally) its gradient.
 * Replaces: classic_ctc_loss / simplified_ctc_loss forward (classic_ctc_loss.py:33-70,
 * simplified_ctc_loss.py:32-67 -> base_loss.py:38-99 -> loss_data.loss) and the first-order backward
 * forward_fn.backprop = d_loss[:,None,None] * gradient (base_loss.py:140-155, 262-298) composed with TF's
 * autodiff of log_softmax (tools.py:37-39) when wrt == CTC_AMD_WRT_LOGITS.
 *   grad   may be NULL (loss only).
 *   d_loss may be NULL (== ones); otherwise [B] upstream gradient that scales each sample's gradient.
 */
int ctc_amd_loss_grad(int kind, int wrt,
                      const float *logits, const int32_t *labels, int label_stride,
                      const int32_t *label_length, const int32_t *logit_length, int blank_index,
                      int B, int T, int V, int U,
                      float *loss, float *grad, const float *d_loss,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * Forward/backward lattice variables in the reference's own layout and units (natural log, -inf for
 * impossible states): classic alpha/beta[B][T+1][U+1][2] (s=0 closed, s=1 open), simplified [B][T+1][U+1].
 * Replaces: ClassicCtcLossData.alpha/.beta (classic_ctc_loss.py:310-462), SimplifiedCtcLossData.alpha/.beta
 * (simplified_ctc_loss.py:291-438).  Parity/debug entry point; not on the fast path.
 * Here U must equal max(label_length) for the shapes to match the reference's.
 */
int ctc_amd_alpha_beta(int kind, int wrt,
                       const float *logits, const int32_t *labels, int label_stride,
                       const int32_t *label_length, const int32_t *logit_length, int blank_index,
                       int B, int T, int V, int U,
                       float *loss, float *alpha, float *beta,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * lg[B][T][V] = natural log of the posterior P(frame t emits token k | label) -- minus the gradient w.r.t. log-probabilities,
 * in log space: finite where the float32 gradient has underflowed (a posterior of e^-150 is returned as -150), -inf for
 * tokens no lattice state emits, for frames beyond logit_length and for infeasible samples.  Also writes loss[B].
 * Replaces: loss_data.logarithmic_logproba_gradient (base_loss.py:270-298): the segment log-sum-exp of
 * _combine_transition_probabilities(alpha[:, :-1], beta[:, 1:]) by token (base_loss.py:420-468, tools.py:74-119).
 * Debug / analysis entry point like ctc_amd_alpha_beta (three-kernel pipeline, full lattice rows).  V <= 8192.
 * Workspace: CTC_AMD_WS_ALPHA_BETA.
 */
int ctc_amd_log_posterior(int kind, int wrt,
                          const float *logits, const int32_t *labels, int label_stride,
                          const int32_t *label_length, const int32_t *logit_length, int blank_index,
                          int B, int T, int V, int U,
                          float *loss, float *lg,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Dense Hessian hess[B][T][V][T][V] (the O(l^4) path), plus loss and gradient (grad may be NULL).
 * Replaces: loss_data.hessian (base_loss.py:186-260) for wrt == CTC_AMD_WRT_LOGPROBS, and
 * tape.batch_jacobian(tape.gradient(sum(loss), logits), logits) (README.md:58-71) for
 * wrt == CTC_AMD_WRT_LOGITS.  The reference's gamma tensor (classic_ctc_loss.py:167-308,
 * simplified_ctc_loss.py:85-191) is never materialised.
 */
int ctc_amd_hessian(int kind, int wrt,
                    const float *logits, const int32_t *labels, int label_stride,
                    const int32_t *label_length, const int32_t *logit_length, int blank_index,
                    int B, int T, int V, int U,
                    float *loss, float *grad, float *hess,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * ctc_amd_loss_grad for the formats a producer kernel hands over: logits (and the gradient written back) as float32,
 * bfloat16 or float16 (CTC_AMD_F32 / CTC_AMD_BF16 / CTC_AMD_F16), with arbitrary element strides of the batch and time axes -- time-major [T,B,V] activations are
 * logits_stride_b = V, logits_stride_t = B*V; the token axis is contiguous.  Arithmetic is float32 either way.
 * Replaces: the `logit_to_logproba` entry of ctc_loss (base_loss.py:59, tools.py:27-40), which the reference can only
 * feed with a contiguous float32 [B,T,V] tensor (a transposed or bfloat16 producer pays one more 262 MB pass there).
 * SURVEY.md section 8(f) rank 3.  Workspace: CTC_AMD_WS_LOSS_GRAD.  Strides are in elements and must be >= V.
 */
int ctc_amd_loss_grad_ex(int kind, int wrt,
                         const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                         const int32_t *labels, int label_stride,
                         const int32_t *label_length, const int32_t *logit_length, int blank_index,
                         int B, int T, int V, int U,
                         float *loss, void *grad, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t,
                         const float *d_loss,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * ctc_amd_loss_grad_ex for PACKED (ragged) batches: no padding frames in memory.  Utterance b owns the logit_length[b] rows
 * row_offsets[b] .. row_offsets[b] + logit_length[b] - 1 of a [total_rows][row_stride] tensor (row_stride >= V elements, the
 * token axis contiguous); the gradient has the same packing (and its own element type).  T is max(logit_length) (a bound is
 * fine: it sizes the workspace, CTC_AMD_WS_LOSS_GRAD).  row_offsets is a DEVICE array of B int64; the ranges must not overlap.
 * Rows beyond logit_length[b] do not exist and are neither read nor written.  Runs the three-kernel pipeline.
 * Replaces: the [batch, max_length, num_tokens] padding the reference requires of its caller (base_loss.py:105-138) together
 * with the masks that undo it (base_loss.py:283-298).  SURVEY.md section 8(f) rank 3 (producer formats).
 */
int ctc_amd_loss_grad_packed(int kind, int wrt,
                             const void *logits, int logits_dtype, const int64_t *row_offsets, int64_t row_stride,
                             const int32_t *labels, int label_stride,
                             const int32_t *label_length, const int32_t *logit_length, int blank_index,
                             int B, int T, int V, int U,
                             float *loss, void *grad, int grad_dtype, int64_t grad_row_stride,
                             const float *d_loss,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * ctc_amd_loss_grad_ex that also accumulates what a training loop takes from the losses, without a launch of its own.
 * Replaces: tf.reduce_sum / reduce_mean of the loss over the finite samples (README.md:62, tests/benchmark.py:199).
 *   sum2[0] += sum over the finite loss[b] of round(loss[b] * 2^20)   (int64, fixed point: integer adds give the same
 *              bits whatever order the workgroups finish in -- and whatever order ranks are all-reduced in; a single
 *              loss beyond +-2^42 ~ 4.4e12 enters clamped to that, so that it cannot wrap the sum)
 *   sum2[1] += number of finite loss[b]
 *   sum2 must hold zeros on entry (or a running total the caller wants to extend); zero_next, if not NULL, points at the
 *   two int64 of the NEXT step and is cleared by this call -- alternate two buffers and nothing ever needs a memset.
 * The linear-domain fused kernel adds inside its one launch; the other pipelines append one small launch.
 * Everything else as ctc_amd_loss_grad_ex.
 */
int ctc_amd_loss_grad_sum(int kind, int wrt,
                          const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                          const int32_t *labels, int label_stride,
                          const int32_t *label_length, const int32_t *logit_length, int blank_index,
                          int B, int T, int V, int U,
                          float *loss, void *grad, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t,
                          const float *d_loss, long long *sum2, long long *zero_next,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * First half of a forward -> backward pair (ABI v5): the losses alone, for a caller that WILL ask for the gradient of the same
 * batch with ctc_amd_grad_resume (torch.autograd: forward now, backward once d_loss is known).
 * Replaces: forward_fn (base_loss.py:140-149) when a backward pass follows.
 * Same work and same workspace contents as ctc_amd_loss_grad_ex with grad == NULL.  The difference is which utterances the
 * linear-domain kernel hands to its log-domain roles.  A loss-only call has no posterior mass to check its sweeps against; a
 * stand-alone one (ctc_amd_loss_grad* with grad == NULL: inference, scoring) therefore sends every utterance that shows one of
 * the kernel's conservative signs there -- which includes every utterance with logits as sharp as a trained model's (D7).  This
 * call trusts the linear sweeps' loss only where the sound detector (the posterior mass check of calls with a gradient) finds
 * nothing to redo -- at least 64 frames to spare over what the labels need, at most 12 frames per label position, P decaying by at
 * most 10 bits per frame (11.75 on the simplified lattice: logits up to about N(0, 3.25^2) over 256 tokens), one or two label
 * positions per lane (U <= 128) -- and keeps every sign outside those bounds.  Every loss-only call, stand-alone or first half, also
 * takes the log-domain roles for an utterance with more than 40 frames per label position when lanes hold two or more label
 * positions (U > 64; flag 2048).  The resume
 * call checks every utterance's posterior mass and redoes what fails, so the gradient is always verified; the loss of a
 * non-binding utterance is taken from the linear sweeps as it stands (measured: tests/tools/flag_stats.py).
 * Shapes that do not run the linear-domain fused kernel behave exactly like ctc_amd_loss_grad_ex with grad == NULL.
 * Workspace: CTC_AMD_WS_LOSS_GRAD (or CTC_AMD_WS_LOSS_GRAD_LOGITS), to be handed to ctc_amd_grad_resume untouched.
 */
int ctc_amd_loss_forward(int kind, int wrt,
                         const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                         const int32_t *labels, int label_stride,
                         const int32_t *label_length, const int32_t *logit_length, int blank_index,
                         int B, int T, int V, int U,
                         float *loss,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * Second half of a forward -> backward pair: the gradient for a loss that ctc_amd_loss_forward (or ctc_amd_loss_grad /
 * ctc_amd_loss_grad_ex with grad == NULL) has just computed, weighted by d_loss (which a training loop only knows once the backward pass runs).
 * Replaces: forward_fn.backprop (base_loss.py:150-153) when the forward pass has already run.
 * The loss-only call stops where the alpha and beta chains meet and leaves its checkpoints, the softmax statistics and
 * log P in the workspace; this call runs the remaining half of the same kernel from there (together: one loss+gradient
 * call's work, split over two launches).  Contract: same arguments as that loss-only call, same workspace, nothing else
 * written to the workspace in between.  `loss` is rewritten with the same values for the utterances that the log-domain
 * kernel redoes (normally none).  Shapes that do not run the linear-domain fused kernel ("fused6") compute loss and
 * gradient anew, so the call is always valid after ANY loss-only call with the same arguments.
 * Workspace: CTC_AMD_WS_LOSS_GRAD.
 */
int ctc_amd_grad_resume(int kind, int wrt,
                        const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                        const int32_t *labels, int label_stride,
                        const int32_t *label_length, const int32_t *logit_length, int blank_index,
                        int B, int T, int V, int U,
                        float *loss, void *grad, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t,
                        const float *d_loss,
                        void *workspace, size_t workspace_bytes, void *stream);

/*
 * Hessian-vector product  out[b,t,k] = sum_{t2,k2} H[b,t,k,t2,k2] * vec[b,t2,k2]  without materialising H
 * (H as ctc_amd_hessian would fill it for the same `wrt`).  O(T*U) memory and work per utterance (tangent-mode
 * alpha/beta recursion), so it works at sizes where the [B,T,V,T,V] tensor does not fit.
 * Replaces: gradient_fn.backprop (base_loss.py:157-175), i.e. the contraction the reference performs with a
 * materialised Hessian when the gradient is differentiated once more (README.md:58-71).
 *   vec, out  [B,T,V] float   (H is symmetric, so this is also vec^T H)
 *   loss      [B] (out), grad [B,T,V] (out, NULL to skip): as ctc_amd_hessian
 * Workspace: CTC_AMD_WS_HVP.
 */
int ctc_amd_hvp(int kind, int wrt,
                const float *logits, const int32_t *labels, int label_stride,
                const int32_t *label_length, const int32_t *logit_length, int blank_index,
                int B, int T, int V, int U,
                const float *vec, float *loss, float *grad, float *out,
                void *workspace, size_t workspace_bytes, void *stream);

/*
 * Best-path (Viterbi) forced alignment, ABI v6: which frame emits which label.  The lattice of the loss in the (max, +)
 * semiring: over the paths pi in [0, V)^T_b (T_b = logit_length[b]) that give labels[b, :label_length[b]] -- classic: after
 * collapsing repeats, then dropping blanks; simplified: after dropping blanks only -- the one that maximises
 * sum_t lp[b, t, pi_t], lp = log_softmax(logits) (CTC_AMD_WRT_LOGPROBS: the input as it stands).
 * The reference has no counterpart (it answers "how probable", base_loss.py:38-99, not "where").
 *   score[B]            float32: the maximum; -inf when no path exists
 *   tokens[B][T]        int32:   pi_t; -1 for t >= T_b
 *   label_index[B][T]   int32:   index into labels[b] of the label the frame emits (classic: or continues by repeating it),
 *                                -1 on blank frames and for t >= T_b.  May be NULL.
 * An infeasible utterance (too few frames, no path of finite value, or infeasible by the input contract, DESIGN.md
 * section 5.8) gets score = -inf and -1 in every frame.  label_length == 0: the all-blank path.  T_b == 0: score 0 for an empty
 * label, -inf otherwise.  Among paths of equal value the choice is deterministic (the same bits every run) but unspecified.
 * The recursion runs on the raw logits in float64, so the path is the exact optimum of the float32 inputs; the error of
 * `score` is that of the float32 row log-sum-exps (none for CTC_AMD_WRT_LOGPROBS) plus its own rounding.
 * Logits in the producer formats of ctc_amd_loss_grad_ex (element type, element strides >= V, token axis contiguous).
 * Workspace: ctc_amd_best_path_workspace_bytes (back-pointers: 64 to 512 bytes per frame) -- a query of its own, the
 * selectors of ctc_amd_workspace_bytes are unchanged.  One launch, asynchronous on `stream`, capturable.
 */
int ctc_amd_best_path_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes /*host*/);
int ctc_amd_best_path(int kind, int wrt,
                      const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                      const int32_t *labels, int label_stride,
                      const int32_t *label_length, const int32_t *logit_length, int blank_index,
                      int B, int T, int V, int U,
                      float *score, int32_t *tokens, int32_t *label_index /* may be NULL */,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * Greedy decoding (added under ABI v6: two new entry points, nothing existing changed): which label sequence the model emits.
 * The frame-wise argmax path -- the unconstrained optimum of sum_t lp[b, t, pi_t], lp = log_softmax(logits)
 * (CTC_AMD_WRT_LOGPROBS: the input as it stands) -- and the label sequence it stands for under the collapse of `kind`.
 * The reference has no counterpart.  No labels are passed in.  T_b = logit_length[b] clamped to [0, T].
 *   tokens[B][T]          int32:   tokens[b, t] = the LOWEST k with x[b, t, k] = max_k x[b, t, k] (values compared as the float32
 *                                  the element type converts to; ties go to the lowest token index: specified, unlike the tie
 *                                  rule of ctc_amd_best_path); -1 for t >= T_b
 *   score[B]              float32: sum_{t < T_b} lp[b, t, tokens[b, t]], accumulated in float64; 0 for T_b == 0.  A frame whose
 *                                  maximum is -inf makes it -inf (tokens is still the lowest index, the call completes normally).
 *   decoded[B][T]         int32:   tokens[b, :T_b] collapsed -- CTC_AMD_CLASSIC: equal neighbours merged, then blanks dropped;
 *                                  CTC_AMD_SIMPLIFIED: blanks dropped only (every non-blank frame is a label); -1 beyond
 *                                  decoded_length[b].  There is no U: a decoding has at most T_b labels, hence the width T.
 *   decoded_length[B]     int32
 *   frames[B][T]          int32:   first frame of each decoded label, -1 padding.  May be NULL.
 *   label_score[B][T]     float32: sum of lp over the run of each decoded label, in time order in float64 -- classic: the unbroken
 *                                  repeat of that token starting at frames[b, i]; simplified: that one frame -- -inf padding.
 *                                  Blank frames count towards `score` only.  May be NULL.
 * decoded / decoded_length can be handed to ctc_amd_loss_grad* and ctc_amd_best_path as labels / label_length
 * (label_stride = T) while decoded_length <= CTC_AMD_MAX_U.  Results for NaN inputs are unspecified (the call completes).
 * 0 <= blank_index < V; no vocabulary limit (no row is staged in LDS).  Logits in the producer formats of ctc_amd_loss_grad_ex
 * (element type, element strides >= V, token axis contiguous): 16-byte (float32) / 8-byte (16-bit types) row accesses when V,
 * the strides and the base pointer allow them, element-wise accesses with identical results otherwise.
 * Workspace: ctc_amd_greedy_decode_workspace_bytes (the float32 lp[B][T], rounded up to 256 bytes).  Two launches (frame-parallel
 * row statistics, then one wavefront per utterance for the collapse), asynchronous on `stream`, capturable.
 */
int ctc_amd_greedy_decode_workspace_bytes(int B, int T, size_t *out_bytes /*host*/);
int ctc_amd_greedy_decode(int kind, int wrt,
                          const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                          const int32_t *logit_length, int blank_index, int B, int T, int V,
                          float *score, int32_t *tokens, int32_t *decoded, int32_t *decoded_length,
                          int32_t *frames /* may be NULL */, float *label_score /* may be NULL */,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Prefix beam search (added under ABI v6: two new entry points, nothing existing changed): the most probable label sequences,
 * each summed over its alignments inside the beam.  The reference has no counterpart.  No labels are passed in.
 * T_b = logit_length[b] clamped to [0, T]; lp = log_softmax(logits) (CTC_AMD_WRT_LOGPROBS: the input as it stands).
 *   Candidates of a frame: the blank, and the min(top_k, V - 1) non-blank tokens with the largest x[b, t, k] (values compared as
 *   the float32 the element type converts to, ties to the lowest index -- the rule of ctc_amd_greedy_decode).  A non-blank token
 *   outside the cut is not considered at that frame, neither to extend a prefix nor to repeat its last label.
 *   CTC_AMD_CLASSIC: a hypothesis is a prefix y with the masses pb (paths ending in blank) and pnb (paths ending in y's last label
 *   e), starting from the empty prefix with pb = 1.  Per frame, with tot = pb + pnb: y keeps pb' += tot * p[blank] and, if e is a
 *   candidate, pnb' += pnb * p[e]; y + c gets pnb' += (c == e ? pb : tot) * p[c] for every non-blank candidate c.
 *   CTC_AMD_SIMPLIFIED: one mass per prefix; y keeps p' += p * p[blank], y + c gets p' += p * p[c].
 *   Contributions to the same prefix add, on both lattices (an extension that meets a hypothesis already in the beam).
 *   Hypotheses of zero mass are dropped; of the rest the beam_width of largest total mass survive the frame.  After the last
 *   frame they are ordered by total mass, descending; among equal masses the choice is deterministic but unspecified.
 *   score[B][nbest]            float32: ln of the hypothesis' total mass; -inf for a missing hypothesis (fewer alive than nbest)
 *   decoded[B][nbest][T]       int32:   its labels, -1 beyond decoded_length (a missing hypothesis: all -1)
 *   decoded_length[B][nbest]   int32
 * T_b == 0 gives one hypothesis, the empty one, with score 0.  A frame whose every candidate is -inf kills the whole beam.
 * Results for NaN inputs are unspecified (the call completes).  decoded[b][n] / decoded_length[b][n] can be handed to
 * ctc_amd_loss_grad* and ctc_amd_best_path as labels / label_length (label_stride = nbest * T) while decoded_length <= CTC_AMD_MAX_U.
 * The masses are linear-domain float64 relative to the row maxima (rescaled by exact powers of two), so the ranking is that of a
 * float64 evaluation of the definition up to reassociation; the error of `score` is that of the float32 row log-sum-exps (none
 * for CTC_AMD_WRT_LOGPROBS) plus its own rounding.  Assumption: two prefixes are taken for the same one when their 64-bit
 * hashes (of the whole label sequence) are equal; a collision among the at most 64 prefixes of a beam would merge two
 * hypotheses silently (about 2^-52 per frame at full width), and is not detected.
 * 1 <= beam_width <= CTC_AMD_BEAM_MAX_WIDTH, 1 <= top_k <= CTC_AMD_BEAM_MAX_TOP_K, 1 <= nbest <= beam_width, 0 <= blank_index < V,
 * V <= CTC_AMD_MAX_V.  Logits in the producer formats of ctc_amd_loss_grad_ex, with the access paths of ctc_amd_greedy_decode.
 * Workspace: ctc_amd_beam_search_workspace_bytes (per frame 16 + 8 * min(top_k, V - 1) bytes of candidates, per utterance
 * 8 * (1 + beam_width * T) bytes of prefix trie).  Two launches (frame-parallel candidate selection, then one wavefront per
 * utterance for the search), asynchronous on `stream`, capturable.
 */
#define CTC_AMD_BEAM_MAX_WIDTH 64
#define CTC_AMD_BEAM_MAX_TOP_K 32
int ctc_amd_beam_search_workspace_bytes(int B, int T, int V, int beam_width, int top_k, size_t *out_bytes /*host*/);
int ctc_amd_beam_search(int kind, int wrt,
                        const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                        const int32_t *logit_length, int blank_index, int B, int T, int V,
                        int beam_width, int top_k, int nbest,
                        float *score, int32_t *decoded, int32_t *decoded_length,
                        void *workspace, size_t workspace_bytes, void *stream);

/*
 * N-best rescoring (added under ABI v6: two new entry points, nothing existing changed): the exact loss of N label sequences
 * per utterance, summed over ALL alignments (the scores of ctc_amd_beam_search are sums inside the beam: lower bounds).
 *   loss[b, n] = -ln P(labels[b, n, :label_length[b, n]] | logits[b])        float32 [B][N]
 * on the lattice of `kind`, with lp = log_softmax(logits) (CTC_AMD_WRT_LOGPROBS: the input as it stands).  It replaces nothing in
 * the reference, which has no counterpart; it replaces N calls of ctc_amd_loss_grad_ex (grad = NULL) on N copies of the logits.
 * Hypothesis (b, n) lies at labels + (b * N + n) * label_stride, its length at label_length[b * N + n]: the layout
 * ctc_amd_beam_search writes (decoded[B][nbest][T] with label_stride = T, decoded_length[B][nbest]).  Every utterance's logits
 * rows are read once per group of CTC_AMD_NBEST_GROUP hypotheses.  Forward only: there is no gradient.
 * Padding and edges, per hypothesis (the input contract of every entry point): labels beyond
 * label_length are not read (the -1 padding of the beam search included); label_length <= 0 is the all-blank path; a label
 * position beyond label_stride reads as the blank; a label outside [0, V) or equal to blank_index inside label_length, a
 * label_length > U, too few frames and a path set of zero mass (-inf log-probabilities, a frame that is -inf everywhere) all
 * give loss = +inf for THAT hypothesis and change nothing else.  T_b = logit_length[b] clamped to [0, T]; frames beyond it are not
 * read; T_b == 0 gives 0 for an empty hypothesis and +inf otherwise.  B == 0 returns CTC_AMD_OK without a launch.
 * loss[b, n] has the same bits whatever N is, whatever the other hypotheses are and wherever in the list it stands.
 * Results for NaN and +inf inputs are unspecified (the call completes).
 * The lattice state is the float64 logarithm of the forward mass (nothing is rescaled, so nothing can be flushed); the error of
 * `loss` is that of the float32 row log-sum-exps (none for CTC_AMD_WRT_LOGPROBS) and of the float32 exp / log of float64
 * differences on the chain, about 1e-7 per frame and unbiased, plus its own rounding.
 * 1 <= N <= CTC_AMD_NBEST_MAX, B * N < 2^31, U <= CTC_AMD_MAX_U bounds every hypothesis, 0 <= blank_index < V,
 * V <= CTC_AMD_MAX_V (no row is staged in LDS; the limit is the ABI's, kept uniform).  Logits in the producer formats of
 * ctc_amd_loss_grad_ex (element type, element strides >= V, token axis contiguous): 16-byte (float32) / 8-byte (16-bit types) row
 * accesses when V, the strides and the base pointer allow them, element-wise accesses with identical results otherwise.
 * Workspace: none.  ctc_amd_nbest_loss_workspace_bytes returns 0 for every valid shape (it exists so that a caller written
 * against it keeps working should that change) and `workspace` may be NULL.  One launch of B * ceil(N / CTC_AMD_NBEST_GROUP)
 * workgroups, asynchronous on `stream`, capturable.
 */
#define CTC_AMD_NBEST_MAX 64   /* = CTC_AMD_BEAM_MAX_WIDTH */
#define CTC_AMD_NBEST_GROUP 8  /* hypotheses that share one read of the logits */
int ctc_amd_nbest_loss_workspace_bytes(int kind, int B, int T, int V, int U, int N, size_t *out_bytes /*host*/);
int ctc_amd_nbest_loss(int kind, int wrt,
                       const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                       const int32_t *labels, int label_stride,
                       const int32_t *label_length /* [B][N] */, const int32_t *logit_length, int blank_index,
                       int B, int T, int V, int U, int N,
                       float *loss /* [B][N] */,
                       void *workspace /* may be NULL */, size_t workspace_bytes, void *stream);

/*
 * Gradient of N-best rescoring (added under ABI v6: two new entry points, nothing existing changed): what MWER-style training
 * (minimum word error rate, expected risk over a beam) needs, without N copies of the logits and N gradient tensors.  With
 * loss[b, n] exactly as ctc_amd_nbest_loss defines it (the SAME BITS for the same inputs; it is written as well) and x the logits:
 *   grad[b, t, k] = sum over the n with a finite loss[b, n] of  weight[b, n] * d loss[b, n] / d x[b, t, k]        for t < T_b
 *                 = sum_n' weight[b, n] * (softmax(x[b, t])[k] - gamma_n[t, k])                   CTC_AMD_WRT_LOGITS
 *                 = - sum_n' weight[b, n] * gamma_n[t, k]                                         CTC_AMD_WRT_LOGPROBS
 *   grad[b, t, :] = 0 exactly                                                                     for T_b <= t < T
 * gamma_n[t, k] is the posterior that frame t emits token k given hypothesis n.  A hypothesis whose loss is +inf (infeasible,
 * malformed, too long, too few frames, zero mass) contributes exactly zero and its weight[b, n] is NOT INTERPRETED: it may be NaN
 * or infinite (what the backward of a `where` / logsumexp in front of the call hands down).  An utterance without a feasible
 * hypothesis gets a zero gradient.  The weights of feasible hypotheses must be finite.
 *   weight[B][N] float32 (in), loss[B][N] float32 (out), grad (out) of element type grad_dtype in {CTC_AMD_F32, CTC_AMD_BF16,
 *   CTC_AMD_F16} with element strides grad_stride_b / grad_stride_t >= V, token axis contiguous: every row t < T of every utterance
 *   is written, elements between V and the stride are not.  All three must be non-NULL when B > 0 (CTC_AMD_EINVAL; a caller who
 *   wants the loss alone has ctc_amd_nbest_loss).
 * Inputs, padding, edges, limits and validation are those of ctc_amd_nbest_loss (checked in the same order; the gradient's element
 * type and strides are checked with the logits'); in addition B * T < 2^33 (the row stage's launch grid).  B == 0 returns
 * CTC_AMD_OK without a launch.
 * The same bits on every run: the posteriors of a row are summed as 64-bit integers in units of 2^(e - 40), 2^e > max_n
 * |weight[b, n]| over the feasible hypotheses, so no order of arrival enters; no floating-point atomics anywhere.
 * Numerics: the alpha and beta sweeps carry float64 base-2 logarithms, as ctc_amd_nbest_loss; a posterior is the float32 exp2 of a
 * float64 difference; the softmax comes from the float32 row statistics.
 * Workspace (may hold anything on entry; too small: CTC_AMD_EWORKSPACE before any launch), with S = 2 (classic) or 1 (simplified),
 * NL the smallest power of two with 64 * NL >= U (1 for U <= 64) and r256(x) = x rounded up to a multiple of 256:
 *   ctc_amd_nbest_loss_grad_workspace_bytes = r256(8 * B * N * T * (S * 64 * NL + 2)) + r256(16 * B * T) + r256(8 * B * N)
 * -- every chain's float64 state of every frame (overwritten by the posteriors), the row statistics, log2 P.  B = 256, T = 1000,
 * U = 128, N = 8: 4.23 GB classic, 2.13 GB simplified (section 7 names what would cut it).
 * Three launches (T == 0: one): the alpha sweep that keeps its rows and the beta sweep, B * ceil(N / CTC_AMD_NBEST_GROUP) workgroups
 * each, then one wavefront per row (b, t).  No allocation, copy or synchronisation; asynchronous on `stream`, capturable.
 */
int ctc_amd_nbest_loss_grad_workspace_bytes(int kind, int B, int T, int V, int U, int N, size_t *out_bytes /*host*/);
int ctc_amd_nbest_loss_grad(int kind, int wrt,
                            const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                            const int32_t *labels, int label_stride,
                            const int32_t *label_length /* [B][N] */, const int32_t *logit_length, int blank_index,
                            int B, int T, int V, int U, int N,
                            const float *weight /* [B][N] */, float *loss /* [B][N] */,
                            void *grad, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * N-best forced alignment (added under ABI v6: two new entry points, nothing existing changed): where each of N label sequences
 * per utterance lies in time.  What N calls of ctc_amd_best_path on labels + n * label_stride would give, from one read of the
 * logits per group of CTC_AMD_NBEST_GROUP hypotheses and with eight chains per workgroup.  Hypothesis (b, n) lies at
 * labels + (b * N + n) * label_stride, its length at label_length[b * N + n]: the layout ctc_amd_beam_search writes and
 * ctc_amd_nbest_loss reads.  Per hypothesis, for the utterance logits[b]:
 *   score[B][N]             float32: as ctc_amd_best_path documents it; -inf when no path exists
 *   tokens[B][N][T]         int32:   as ctc_amd_best_path: pi_t, -1 for t >= T_b
 *   label_index[B][N][T]    int32:   as ctc_amd_best_path: -1 on blank frames and for t >= T_b.  May be NULL.
 *   first_frame[B][N][U]    int32:   the first frame whose label_index is i, for i < label_length[b, n]; -1 for
 *   last_frame[B][N][U]     int32:   label_length[b, n] <= i < U.  ... and the last.  On the simplified lattice the two are equal.
 *                                    Each may be NULL.
 * An infeasible hypothesis gets score = -inf and -1 in every frame and label, and changes nothing else.  The infeasible cases
 * are those of ctc_amd_nbest_loss: too few frames, label_length > U, a label outside [0, V) or equal to blank_index inside
 * label_length, a label position beyond label_stride, no path of finite value.  label_length <= 0 is the all-blank path; labels
 * beyond label_length are not read.  T_b = logit_length[b] clamped to [0, T]; frames beyond it are not read; T_b == 0 gives score 0
 * for an empty hypothesis and -inf otherwise.  B == 0 returns CTC_AMD_OK without a launch.
 * Every output of (b, n) has the same bits whatever N is, whatever the other hypotheses are and wherever in the list it stands,
 * and on every run: no floating-point atomics anywhere, every element has one writer.
 * Ties: among paths of equal float64 value the choice is deterministic but unspecified, in the words of ctc_amd_best_path.  That
 * is the guarantee.  The recursion, its candidate order and its strict comparisons are those of ctc_amd_best_path, so in practice
 * the path is the one that call chooses; the tests hold the two equal on random inputs, the ABI does not promise it.  `score` may
 * differ from ctc_amd_best_path's in its last bits (the float64 sum of the rows' log-sum-exps is taken in another order).
 * Results for NaN and +inf inputs are unspecified (the call completes).
 * Limits and validation are those of ctc_amd_nbest_loss, checked in the same order: 1 <= N <= CTC_AMD_NBEST_MAX, B * N < 2^31,
 * U <= CTC_AMD_MAX_U, 0 <= blank_index < V, V <= CTC_AMD_MAX_V (no row is staged in LDS), the producer formats of
 * ctc_amd_loss_grad_ex with both access paths; then score and tokens must be non-NULL (CTC_AMD_EINVAL), then the workspace.
 * Workspace (may hold anything on entry; too small: CTC_AMD_EWORKSPACE before any launch): the back-pointers alone.  With NL the
 * smallest power of two with 64 * NL >= U (1 for U <= 64), word = 1, 1, 2, 4, 8 bytes for NL = 1, 2, 4, 8, 16 and r256(x) = x
 * rounded up to a multiple of 256:
 *   ctc_amd_nbest_best_path_workspace_bytes = r256(B * N * T * 64 * word)
 * B = 256, T = 1000, U = 128, N = 8: 131 MB.  One launch of B * ceil(N / CTC_AMD_NBEST_GROUP) workgroups (sweep and back-trace
 * in the same kernel), asynchronous on `stream`, capturable.  No allocation, copy or synchronisation.
 */
int ctc_amd_nbest_best_path_workspace_bytes(int kind, int B, int T, int V, int U, int N, size_t *out_bytes /*host*/);
int ctc_amd_nbest_best_path(int kind, int wrt,
                            const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                            const int32_t *labels, int label_stride,
                            const int32_t *label_length /* [B][N] */, const int32_t *logit_length, int blank_index,
                            int B, int T, int V, int U, int N,
                            float *score /* [B][N] */, int32_t *tokens /* [B][N][T] */,
                            int32_t *label_index /* [B][N][T], may be NULL */,
                            int32_t *first_frame /* [B][N][U], may be NULL */, int32_t *last_frame /* [B][N][U], may be NULL */,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * Edit distance of N-best lists (added under ABI v6: two new entry points, nothing existing changed): the Levenshtein distance --
 * unit cost for insertion, deletion and substitution -- of every hypothesis to its utterance's reference transcript, the risk of
 * MWER-style training (minimum word error rate: expected risk over a beam) and the numerator of a token error rate.
 *   distance[b, n] = D(hyp[b, n, :h], ref[b, :r])                                int32 [B][N], exact
 * Hypothesis (b, n) lies at hyp + (b * N + n) * hyp_stride, its length at hyp_length[b * N + n]: the layout ctc_amd_beam_search
 * writes (decoded[B][nbest][T] with hyp_stride = T, decoded_length[B][nbest]) and ctc_amd_nbest_loss reads.  The reference of
 * utterance b lies at ref + b * ref_stride, its length at ref_length[b].  It replaces nothing in the reference implementation,
 * which has no counterpart; it replaces a copy of the hypotheses to the host, a dynamic programme there and a copy back.
 * Tokens are arbitrary int32 values compared for equality: there is no vocabulary limit and no blank, so word ids mapped on the host
 * work as well as characters or sub-word units.
 * Lengths: h = hyp_length[b, n] clamped to [0, hyp_stride], r = ref_length[b] clamped to [0, ref_stride]; elements beyond h and r
 * are not read (the -1 padding of the beam search included).  h == 0 gives r and r == 0 gives h.
 * R bounds every reference length, 0 <= R <= CTC_AMD_MAX_U: an utterance with r > R gets distance = -1 for all its hypotheses
 * and changes nothing else (the counterpart of "label_length > U gives +inf").  The hypothesis length has no limit other than the
 * stride, 0 <= hyp_stride <= CTC_AMD_EDIT_MAX_STRIDE.  N >= 1 (no upper limit), B * N < 2^31.  B == 0 returns CTC_AMD_OK without a
 * launch.
 * Validation before any launch (CTC_AMD_EINVAL, ctc_amd_last_error): negative B, R or strides, R or hyp_stride beyond its limit,
 * N < 1, the product limit, then null pointers (hyp / ref may be NULL when their stride is 0).
 * Every element of `distance` has one writer; distance[b, n] is the same whatever N is, whatever the other hypotheses are and
 * wherever in the list it stands, and on every run.
 * Workspace: none.  ctc_amd_edit_distance_workspace_bytes returns 0 for every valid shape (it exists so that a caller written
 * against it keeps working should that change) and `workspace` may be NULL.  One launch of ceil(B * N / 4) workgroups, one
 * wavefront per pair, h + ceil(r / NL) - 1 <= h + 63 sequential steps each with NL the smallest power of two with 64 * NL >= R
 * (DESIGN.md section 5.13); asynchronous on `stream`, capturable, no allocation, copy or synchronisation.
 */
#define CTC_AMD_EDIT_MAX_STRIDE 2147479552 /* 2^31 - 4096: row indices and distances stay inside int32 */
int ctc_amd_edit_distance_workspace_bytes(int B, int N, int R, size_t *out_bytes /*host*/);
int ctc_amd_edit_distance(const int32_t *hyp, int hyp_stride, const int32_t *hyp_length /* [B][N] */,
                          const int32_t *ref, int ref_stride, const int32_t *ref_length /* [B] */,
                          int B, int N, int R,
                          int32_t *distance /* [B][N] */,
                          void *workspace /* may be NULL */, size_t workspace_bytes, void *stream);

/*
 * CTC prefix scores (added under ABI v6: four new entry points, nothing existing changed): the step-wise scorer of
 * label-synchronous decoding (Watanabe et al. 2017, algorithm 2) -- joint CTC / attention decoding, shallow fusion with a
 * language model whose state stays on the caller's side.  It replaces nothing in the reference, which has no counterpart.
 * With lp = log_softmax(logits[b]) (CTC_AMD_WRT_LOGPROBS: the input as it stands), T_b = logit_length[b] clamped to [0, T], k0 the
 * blank and a prefix g of m labels, rn[t] / rb[t] = ln P(frames 0..t emit exactly g and frame t is a label / a blank):
 *   empty prefix   rn[t] = -inf, rb[t] = sum_{tau <= t} lp[tau, k0]
 *   entry weight   phi[0] = 0 if m == 0 else -inf;  phi[t] = lse(rb[t-1], rn[t-1]) for t >= 1, on the classic lattice
 *                  rb[t-1] alone when c == last(g)
 *   prefix score   ln psi(g.c) = lse_{t < T_b}(phi[t] + lp[t, c]): the mass of ALL label sequences that start with g.c
 *   extension      classic rn'[t] = lse(rn'[t-1], phi[t]) + lp[t, c];  simplified rn'[t] = phi[t] + lp[t, c];
 *                  both rb'[t] = lse(rb'[t-1], rn'[t-1]) + lp[t, k0]
 *   full score     ln P(g) = lse(rn[T_b-1], rb[T_b-1]);  T_b == 0: 0 for the empty prefix, -inf otherwise
 * so that psi(g) = P(g) + sum_c psi(g.c).  c == k0 or c outside [0, V) is an impossible emission: score -inf, extension dead.
 *
 * A beam is N hypotheses per utterance in four buffers of the caller: state (float64, ctc_amd_prefix_workspace_bytes'
 * state_bytes = 8 * B * N * (2 * T + 2), opaque), last_token, length (int32 [B][N]; a dead hypothesis has -1 in both) and
 * full_score (float32 [B][N], natural logarithm).
 *   ctc_amd_prefix_rows    the row maximum and log-sum-exp of every frame into `rows` (rows_bytes = 8 * B * T), ONCE per logits
 *                          tensor; the other two calls read them every decoding step.  CTC_AMD_WRT_LOGPROBS needs none: it is not
 *                          called and `rows` may be NULL there.
 *   ctc_amd_prefix_extend  new hypothesis (b, n) = hypothesis (b, parent[b, n]) of the input beam extended by token[b, n].
 *                          parent == -2: the empty prefix (token not read; state_in / last_in / length_in may then be NULL: this is
 *                          how a beam starts); parent == -1, any other parent outside [0, N), a dead parent or an impossible token:
 *                          a dead hypothesis.  parent may repeat and permute; the output buffers must not overlap the input's.
 *   ctc_amd_prefix_score   score[b, n, c] = ln psi(g_{b,n} . c), float32 [B][N][V]: -inf in the blank's column and for a dead
 *                          hypothesis.  The logits are read once per group of CTC_AMD_PREFIX_GROUP hypotheses.
 * Every result of hypothesis (b, n) has the same bits whatever N is, whatever the other hypotheses are and wherever it stands.
 * Numerics as ctc_amd_nbest_loss: float64 state, float32 exp / log of float64 differences, a true -inf, emissions from
 * (double)x - (double)max.  Results for NaN and +inf inputs are unspecified (the calls complete).
 * 1 <= N <= CTC_AMD_PREFIX_MAX, B * N < 2^31, V <= CTC_AMD_MAX_V, 0 <= blank_index < V, logits in the producer formats of
 * ctc_amd_loss_grad_ex.  Checked in the order of ctc_amd_nbest_loss: common arguments, element type, B == 0 (CTC_AMD_OK, no launch),
 * strides, V and N; then null pointers (CTC_AMD_EINVAL) and the buffer sizes (CTC_AMD_EWORKSPACE).
 * One launch each, asynchronous on `stream`, capturable, no allocation, copy or synchronisation.
 */
#define CTC_AMD_PREFIX_MAX 64   /* = CTC_AMD_NBEST_MAX */
#define CTC_AMD_PREFIX_GROUP 8  /* hypotheses that share one read of the logits in ctc_amd_prefix_score */
int ctc_amd_prefix_workspace_bytes(int B, int T, int V, int N, size_t *rows_bytes /*host*/, size_t *state_bytes /*host*/);
int ctc_amd_prefix_rows(const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                        const int32_t *logit_length, int B, int T, int V,
                        void *rows, size_t rows_bytes, void *stream);
int ctc_amd_prefix_extend(int kind, int wrt,
                          const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                          const int32_t *logit_length, int blank_index, int B, int T, int V, int N,
                          const void *rows, size_t rows_bytes,
                          const void *state_in, const int32_t *last_token_in, const int32_t *length_in,
                          const int32_t *parent /* [B][N] */, const int32_t *token /* [B][N] */,
                          void *state_out, size_t state_bytes, int32_t *last_token_out, int32_t *length_out,
                          float *full_score /* [B][N] */, void *stream);
int ctc_amd_prefix_score(int kind, int wrt,
                         const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                         const int32_t *logit_length, int blank_index, int B, int T, int V, int N,
                         const void *rows, size_t rows_bytes,
                         const void *state, size_t state_bytes, const int32_t *last_token, const int32_t *length,
                         float *score /* [B][N][V] */, void *stream);

/*
 * Forced alignment of partial transcripts: wildcard labels (added under ABI v6: two new entry points, nothing existing changed).
 * ctc_amd_best_path forces every frame onto the given labels or the blank; here a label may be a wildcard that takes up whatever
 * else was said: untranscribed speech before, after or inside the known words, a passage the annotator could not make out, the
 * rest of an utterance around a keyword.  The reference has no counterpart.
 *
 * Wildcard value.  One reserved label value, CTC_AMD_WILDCARD = -2, marks a wildcard position.  It applies inside label_length
 * only.  Everything else follows the input contract of the other entry points: any other label outside
 * [0, V) or equal to the blank makes the utterance infeasible; label_length > U makes it infeasible; logit_length is clamped to
 * [0, T] (T_b below).
 * Emission and tokens.  With x the input row (logits, or log-probabilities for CTC_AMD_WRT_LOGPROBS):
 *   m_t = max_k x[t, k] over all tokens, the blank included;
 *   a_t = the lowest k that attains it, compared as the float32 the element type converts to: the tie rule of ctc_amd_greedy_decode.
 * A wildcard position stands for any non-empty run of frames with any tokens on them.  In the (max, +) semiring that run is worth
 * sum m_t, and the tokens reported for it are a_t.
 * Classic lattice.  The recursion of ctc_amd_best_path (open state: the last frame emitted label i; closed state: labels 0..i are
 * done and the last frame was blank) changes as follows for wildcard position i: its emission is m_t; the transition from an open
 * position i - 1 straight into an open wildcard is always allowed, wildcard or not; the transition from an open wildcard i into an
 * open position i + 1 is always allowed, whatever token the wildcard last showed.  Its closed state is the ordinary one.  The
 * frames of a wildcard are therefore contiguous, and each wildcard takes at least one frame.
 * Simplified lattice.  For wildcard position i: entering it costs m_t; while "labels 0..i are emitted" is the current state, the
 * horizontal step costs m_t instead of x[t, blank].  Every frame from the entry until the next label's frame therefore belongs to
 * the wildcard: label_index is i on those frames and tokens is a_t.
 * Labels and edges.  Non-wildcard positions behave exactly as in ctc_amd_best_path.  Adjacent wildcards are allowed, and each
 * takes at least one frame.  Free start and end are a wildcard as the first and last label; there is no separate switch.
 * Score.  score is the maximum of sum_t lp[t, pi_t] over admissible paths, lp = x - LSE_t for logits and x as it stands for
 * log-probabilities, with pi_t = a_t on wildcard frames.  Among paths of equal value the choice is deterministic (the same bits
 * every run) but unspecified, in the words of ctc_amd_best_path.
 * Degenerate cases.  label_length == 0: the all-blank path.  T_b == 0: score 0 for an empty label, -inf otherwise.  An infeasible
 * utterance (also: fewer frames than the positions need -- a wildcard needs a frame of its own): score -inf, and -1 (or -inf)
 * everywhere.  A row that is -inf throughout makes every path through it -inf.  NaN and +inf inputs: unspecified, the call completes.
 *
 *   score[B]            float32
 *   tokens[B][T]        int32:   pi_t; -1 for t >= T_b
 *   label_index[B][T]   int32:   as ctc_amd_best_path documents it; i on every frame of wildcard i, including frames where a_t
 *                                happens to be the blank.  May be NULL.
 *   first_frame[B][U]   int32:   the first frame whose label_index is i, for i < label_length; -1 from label_length on (the
 *   last_frame[B][U]    int32:   convention of ctc_amd_nbest_best_path).  ... and the last.  Each may be NULL.
 *   label_score[B][U]   float32: the sum of lp over the frames whose label_index is i, taken in time order in float64; -inf from
 *                                label_length on and for an infeasible utterance.  Blank frames outside any label count towards
 *                                score only: sum_i label_score + sum over those frames of lp[t, blank] = score.  May be NULL.
 * The recursion runs on the raw inputs in float64, so the path is the exact optimum of the float32 inputs; the error of score and
 * label_score is that of the float32 row log-sum-exps (none for CTC_AMD_WRT_LOGPROBS) plus the rounding of the outputs.
 * Validation and limits are those of ctc_amd_best_path, in its order and with its messages: common arguments (kind, wrt, sizes,
 * 0 <= blank_index < V, U <= CTC_AMD_MAX_U, null pointers), element type, B == 0 (CTC_AMD_OK without a launch), strides, then
 * score and tokens non-NULL, V <= CTC_AMD_MAX_V (CTC_AMD_EINVAL each), then the workspace (CTC_AMD_EWORKSPACE before any launch).
 * Logits in the producer formats of ctc_amd_loss_grad_ex, read in place with both access paths (16-byte / 8-byte row accesses
 * when V, the strides and the base pointer allow them, element-wise with identical results otherwise).
 * Workspace (may hold anything on entry): the back-pointers of ctc_amd_best_path, the float64 log-probability of the path's token
 * on every frame and the int32 a_t of every frame.  With NL the smallest power of two with 64 * NL >= U (1 for U <= 64),
 * word = 1, 1, 2, 4, 8 bytes for NL = 1, 2, 4, 8, 16 and r256(x) = x rounded up to a multiple of 256:
 *   ctc_amd_wildcard_best_path_workspace_bytes = r256(B * T * 64 * word) + r256(B * T * 8) + r256(B * T * 4)
 * B = 256, T = 1000, U = 128: 19.5 MB.  One launch of B workgroups (row pass, sweep, back-trace and the per-label sums in the same
 * kernel), asynchronous on `stream`, capturable.  No allocation, copy or synchronisation.  Every element has one writer, there
 * are no floating-point atomics: the same bits on every run.
 */
#define CTC_AMD_WILDCARD (-2)
int ctc_amd_wildcard_best_path_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes /*host*/);
int ctc_amd_wildcard_best_path(int kind, int wrt,
                               const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                               const int32_t *labels, int label_stride,
                               const int32_t *label_length, const int32_t *logit_length, int blank_index,
                               int B, int T, int V, int U,
                               float *score, int32_t *tokens, int32_t *label_index /* may be NULL */,
                               int32_t *first_frame /* [B][U], may be NULL */, int32_t *last_frame /* [B][U], may be NULL */,
                               float *label_score /* [B][U], may be NULL */,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * Long-form forced alignment: transcripts beyond CTC_AMD_MAX_U labels (added under ABI v6: two new entry points, nothing existing
 * changed; CTC_AMD_MAX_U and every other call's validation stay as they are).  The best path of ctc_amd_best_path -- the same
 * lattices, recursion, candidate order, strict comparisons and float64 state -- for U <= CTC_AMD_LONG_MAX_U label positions: a
 * whole recording against its transcript (ten minutes at 20 ms frames and character labels: T = 30 000, U = 8 000).  The
 * reference has no counterpart.
 *
 * Decomposition.  The lattice is tiled over label blocks of 1024 positions (16 per lane of one
 * wavefront) and time blocks of frames_per_tile frames; K = max(1, ceil(U / 1024)) label blocks, J = max(1, ceil(T / TF)) time
 * blocks.  Launch d = 0 .. K + J - 2 runs the tiles (k, j) with k + j = d of every utterance, one workgroup each; a tile takes its
 * chain state from the row its predecessor in time left and its left edge from the column its left neighbour stored, both on
 * launch d - 1, so the order of the launches on the stream is the only dependency: no workgroup waits for another.  One further
 * launch traces the path back across the tiles, and one more derives first_frame / last_frame when either is asked for.
 * K + J - 1 (+ 1 or 2) launches whatever the lengths are: asynchronous on `stream`, capturable, no allocation, copy or
 * synchronisation.  Vector stores only, no atomics, one writer per element: the same bits on every run.  float64 max and add hand
 * over exactly between tiles, so the path does not depend on frames_per_tile or on B; `score` may differ in its last bits between
 * values of frames_per_tile (the float64 sum of the rows' log-sum-exps is taken per time block, then over the blocks).
 *
 * frames_per_tile: 0 selects CTC_AMD_LONG_FRAMES_DEFAULT; otherwise a positive multiple of CTC_AMD_LONG_FRAMES_MULTIPLE (the
 * frames of one ring block at 16 positions per lane); anything else is CTC_AMD_EINVAL.  Smaller tiles put more workgroups on a
 * diagonal and cost more launches.
 *
 *   score[B]            float32: as ctc_amd_best_path documents it; -inf when no path exists
 *   tokens[B][T]        int32:   pi_t; -1 for t >= T_b
 *   label_index[B][T]   int32:   as ctc_amd_best_path documents it.  May be NULL.
 *   first_frame[B][U]   int32:   the first frame whose label_index is i, for i < label_length; -1 from label_length on (the
 *   last_frame[B][U]    int32:   convention of ctc_amd_nbest_best_path).  ... and the last.  Each may be NULL.
 * The input contract of the other entry points holds: too few frames, label_length > U, a label equal to
 * the blank or outside [0, V) -- CTC_AMD_WILDCARD included: wildcards are not part of this call -- and a position beyond
 * label_stride make the utterance infeasible: score = -inf and -1 everywhere else.  label_length == 0: the all-blank path.
 * T_b == 0: score 0 for an empty label, -inf otherwise.  Ties: deterministic but unspecified, in the words of ctc_amd_best_path;
 * in practice a call with U <= CTC_AMD_MAX_U (legal: one label block) returns the path of ctc_amd_best_path.
 *
 * Validation follows ctc_amd_best_path in its order and with its messages: common arguments (U <= CTC_AMD_LONG_MAX_U in place of
 * CTC_AMD_MAX_U), element type, B == 0 (CTC_AMD_OK without a launch), strides, then score and tokens non-NULL, V <= CTC_AMD_MAX_V,
 * frames_per_tile (also: B so large that a launch grid would pass 2^31 - 1 workgroups) -- CTC_AMD_EINVAL each -- then the
 * workspace (CTC_AMD_EWORKSPACE before any launch).  Logits in the producer formats of ctc_amd_loss_grad_ex, read in place with
 * both access paths (16-byte / 8-byte row accesses when V, the strides and the base pointer allow them, element-wise otherwise).
 *
 * Workspace (may hold anything on entry; every count is a size_t: B * K * T * 512 passes 2^31 at realistic sizes).  With
 * TF = frames_per_tile or the default, K and J as above and r256(x) = x rounded up to a multiple of 256:
 *   ctc_amd_long_best_path_workspace_bytes =
 *       r256(B * K * T * 512)          back-pointers: one 8-byte word per lane, frame and label block
 *     + r256(B * (K - 1) * T * 16)     columns: the float64 pair (open, closed) of a block's last position before every frame
 *     + r256(B * K * 16448)            rows: the chain state of every label block, 2 * 1024 + 8 float64
 *     + r256(B * J * 8)                the log-sum-exp partial sum of every time block
 *     + r256(B * T * 4)                label_index when the caller passes none
 *     + r256(B * 4)                    feasibility of every utterance
 * B = 1, T = 30000, U = 8192, frames_per_tile = 0 (128): K = 8, J = 235:
 *   122 880 000 + 3 360 000 + 131 584 + 2 048 + 120 064 + 256 = 126 493 952 bytes, 242 + 2 launches.
 */
#define CTC_AMD_LONG_MAX_U 65536
#define CTC_AMD_LONG_FRAMES_MULTIPLE 4
#define CTC_AMD_LONG_FRAMES_DEFAULT 128
int ctc_amd_long_best_path_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, size_t *out_bytes /*host*/);
int ctc_amd_long_best_path(int kind, int wrt,
                           const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                           const int32_t *labels, int label_stride,
                           const int32_t *label_length, const int32_t *logit_length, int blank_index,
                           int B, int T, int V, int U, int frames_per_tile,
                           float *score, int32_t *tokens, int32_t *label_index /* may be NULL */,
                           int32_t *first_frame /* [B][U], may be NULL */, int32_t *last_frame /* [B][U], may be NULL */,
                           void *workspace, size_t workspace_bytes, void *stream);

/*
 * Long-form forced alignment of partial transcripts: wildcard labels and per-label scores beyond CTC_AMD_MAX_U labels (added under
 * ABI v6: two new entry points, nothing existing changed).  ctc_amd_wildcard_best_path for U <= CTC_AMD_LONG_MAX_U label
 * positions, computed by the decomposition of ctc_amd_long_best_path: a whole recording against a transcript that leaves out its
 * preface, its applause or its advertisements.  The reference has no counterpart.
 *
 * Semantics are exactly those of ctc_amd_wildcard_best_path (above): a label equal to CTC_AMD_WILDCARD
 * inside label_length is a wildcard position with the definition given there for both lattices; m_t and a_t with the tie rule of
 * ctc_amd_greedy_decode; tokens is a_t on wildcard frames and label_index is i on every frame of wildcard i; label_score is the
 * float64 sum of lp over a label's frames in time order, rounded to float32, and sum_i label_score + the lp of the blank frames
 * outside any label = score; the same degenerate cases; an infeasible utterance (also: fewer frames than the positions need -- a
 * wildcard needs a frame of its own; label_length > U; a label other than the wildcard outside [0, V) or equal to the blank)
 * gives score -inf, -1 in tokens, label_index, first_frame and last_frame and -inf in label_score.  The one difference is
 * U <= CTC_AMD_LONG_MAX_U in place of CTC_AMD_MAX_U.
 *
 *   score[B]            float32
 *   tokens[B][T]        int32:   pi_t; -1 for t >= T_b
 *   label_index[B][T]   int32:   as ctc_amd_wildcard_best_path documents it.  May be NULL.
 *   first_frame[B][U]   int32:   the first frame whose label_index is i, for i < label_length; -1 from label_length on.
 *   last_frame[B][U]    int32:   ... and the last.  Each may be NULL.
 *   label_score[B][U]   float32: as ctc_amd_wildcard_best_path documents it; -inf from label_length on.  May be NULL.
 *
 * Decomposition and launch properties are those of ctc_amd_long_best_path (DESIGN.md sections 5.18, 5.19): label blocks of 1024
 * positions x time blocks of frames_per_tile frames (0: CTC_AMD_LONG_FRAMES_DEFAULT; otherwise a positive multiple of
 * CTC_AMD_LONG_FRAMES_MULTIPLE), K and J as there, one launch per anti-diagonal of tiles, the order of the launches on the stream
 * the only dependency.  The row statistics (m_t, a_t, the log-sum-exp) are taken once, by label block 0, and kept per frame in the
 * workspace for the tiles further right, which run on later launches.  Then one launch traces the path back, one derives
 * first_frame / last_frame when either is asked for and one sums label_score when it is asked for: K + J - 1 (+ 1 .. 3) launches,
 * a number that depends on (T, U, frames_per_tile) and on which outputs are passed, never on the lengths.  Asynchronous on
 * `stream`, capturable, no allocation, copy or synchronisation.  Vector stores only, no atomics, one writer per element: the same
 * bits on every run.  tokens, label_index, first_frame, last_frame and label_score do not depend on frames_per_tile or on B, bit
 * for bit (float64 max and add hand over exactly between tiles; every log-sum-exp is one wavefront's row pass; every label_score
 * is one thread's sum in time order); `score` may differ in its last bits between values of frames_per_tile, as in
 * ctc_amd_long_best_path.
 *
 * Validation follows ctc_amd_long_best_path in its order and with its messages: common arguments (U <= CTC_AMD_LONG_MAX_U),
 * element type, B == 0 (CTC_AMD_OK without a launch), strides, then score and tokens non-NULL, V <= CTC_AMD_MAX_V,
 * frames_per_tile (also: B so large that a launch grid would pass 2^31 - 1 workgroups) -- CTC_AMD_EINVAL each -- then the
 * workspace (CTC_AMD_EWORKSPACE before any launch).  Logits in the producer formats of ctc_amd_loss_grad_ex, read in place with
 * both access paths (identical results).
 *
 * Workspace (may hold anything on entry; every count is a size_t).  The regions of ctc_amd_long_best_path at the same offsets,
 * then three per-frame regions.  With TF, K, J and r256 as there:
 *   ctc_amd_long_wildcard_best_path_workspace_bytes =
 *       r256(B * K * T * 512)          back-pointers: one 8-byte word per lane, frame and label block
 *     + r256(B * (K - 1) * T * 16)     columns: the float64 pair (open, closed) of a block's last position before every frame
 *     + r256(B * K * 16448)            rows: the chain state of every label block, 2 * 1024 + 8 float64
 *     + r256(B * J * 8)                the log-sum-exp partial sum of every time block
 *     + r256(B * T * 4)                label_index when the caller passes none
 *     + r256(B * 4)                    feasibility of every utterance
 *     + r256(B * T * 8)                m_t of every frame, float64
 *     + r256(B * T * 4)                a_t of every frame, int32
 *     + r256(B * T * 8)                the log-sum-exp of every frame, then the log-probability of the path's token, float64
 * B = 1, T = 30000, U = 8192, frames_per_tile = 0 (128): K = 8, J = 235:
 *   122 880 000 + 3 360 000 + 131 584 + 2 048 + 120 064 + 256 + 240 128 + 120 064 + 240 128 = 127 094 272 bytes, 242 + 3 launches.
 */
int ctc_amd_long_wildcard_best_path_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, size_t *out_bytes /*host*/);
int ctc_amd_long_wildcard_best_path(int kind, int wrt,
                                    const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                    const int32_t *labels, int label_stride,
                                    const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                    int B, int T, int V, int U, int frames_per_tile,
                                    float *score, int32_t *tokens, int32_t *label_index /* may be NULL */,
                                    int32_t *first_frame /* [B][U], may be NULL */, int32_t *last_frame /* [B][U], may be NULL */,
                                    float *label_score /* [B][U], may be NULL */,
                                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * CTC loss and gradient with wildcard labels: training on partial transcripts (added under ABI v6: two new entry points, nothing
 * existing changed).  The training-side counterpart of ctc_amd_wildcard_best_path: the same lattice, summed over all its paths
 * instead of maximised, with its analytic gradient.  In the literature: wildcard CTC (W-CTC) and star temporal classification
 * (STC, which adds the per-frame penalty below).  The reference has no counterpart.
 *
 * Labels, lengths, blank, formats and every degenerate case follow the input contract of the other entry points (DESIGN.md section
 * 5.8) and ctc_amd_wildcard_best_path.  A label equal to CTC_AMD_WILDCARD inside label_length marks a wildcard position: any
 * non-empty run of frames with any tokens on them.
 * Emission.  Let lp = log_softmax(x) for CTC_AMD_WRT_LOGITS and x as it stands for CTC_AMD_WRT_LOGPROBS, and w =
 * wildcard_log_weight, a finite float <= 0 (a positive, NaN or infinite w: CTC_AMD_EINVAL).  A wildcard frame emits
 *   e_w(t) = w + ln sum_k exp(lp[t, k])    -- w exactly for logits, w + LSE_k x[t, k] for log-probabilities.
 * The lattices are those of ctc_amd_wildcard_best_path with e_w(t) in place of the row maximum m_t.
 * Classic lattice: 2 L + 1 states.  A wildcard's open state emits e_w; the step from open position i - 1 straight into open
 * position i is allowed when the two labels differ or either is a wildcard; a wildcard's closed state is the ordinary one (blank).
 * The end states are the last two.
 * Simplified lattice: L + 1 states.  Entering label i costs its emission, e_w for a wildcard; staying in the state behind a
 * wildcard costs e_w instead of lp[t, blank].
 * Both: adjacent wildcards take at least one frame each; free start and end are a wildcard as the first and last label.
 *   Z[b] = sum over all state sequences of the product of their emissions,        loss[b] = -ln Z[b]   (float32 [B])
 * Z IS A SUM OVER LATTICE PATHS, NOT A PROBABILITY: one token sequence can match the lattice under several segmentations (a
 * wildcard's frames may show the neighbouring label's token), so Z may exceed 1 and the loss may be negative.  w < 0 is the
 * per-frame penalty STC uses against that.  This is the known property of W-CTC and STC, not a defect.
 * Gradient.  Let gamma_t(k) be the posterior that frame t sits in an ordinary state (label or blank) emitting token k, and Gamma_t
 * the posterior that it sits in a wildcard emission (classic: the wildcard's open state; simplified: the entry into a wildcard or
 * a stay behind one): sum_k gamma_t(k) + Gamma_t = 1.  Then
 *   grad[b, t, k] = d_loss[b] * ((1 - Gamma_t) * softmax(x[b, t])[k] - gamma_t(k))        CTC_AMD_WRT_LOGITS,   t < T_b
 *                 = d_loss[b] * (-gamma_t(k) - Gamma_t * exp(x[b, t, k] - LSE_t))         CTC_AMD_WRT_LOGPROBS, t < T_b
 *                 = 0 exactly                                                              T_b <= t < T
 * Infeasible utterances are those of ctc_amd_wildcard_best_path: too few frames (each wildcard needs a frame of its own),
 * label_length > U, a label outside [0, V) other than CTC_AMD_WILDCARD, a label equal to the blank, a position beyond label_stride,
 * zero mass (also a row that is -inf throughout).  Such an utterance gets loss = +inf and an exactly zero gradient, its d_loss[b]
 * is NOT INTERPRETED (it may be NaN), and it changes nothing else in the batch.  label_length <= 0 is the all-blank path.
 * T_b == 0: loss 0 for an empty transcript, +inf otherwise.  NaN and +inf inputs: unspecified, the call completes.
 * ctc_amd_check_labels keeps rejecting CTC_AMD_WILDCARD: it describes what the plain losses accept.
 *   d_loss[B] float32 (in; NULL = ones), loss[B] float32 (out), grad (out; NULL = forward only, one launch) of element type
 *   grad_dtype with element strides grad_stride_b / grad_stride_t >= V, token axis contiguous: every row t < T of every utterance
 *   is written, elements between V and the stride are not.
 * Validation in the order of ctc_amd_nbest_loss_grad: common arguments, element types, B == 0 (CTC_AMD_OK without a launch),
 * strides (the gradient's only when grad != NULL), then wildcard_log_weight, loss non-NULL, V <= CTC_AMD_MAX_V, B * T < 2^33 when
 * grad != NULL (the row stage's launch grid) (CTC_AMD_EINVAL each), then the workspace (CTC_AMD_EWORKSPACE before any launch).
 * Logits in the producer formats of ctc_amd_loss_grad_ex, read in place with both access paths (16-byte / 8-byte row accesses when
 * V, the strides and the base pointer allow them, element-wise with identical results otherwise).
 * Numerics: the alpha and beta sweeps carry float64 base-2 logarithms, as ctc_amd_nbest_loss; a posterior is the float32 exp2 of a
 * float64 difference; the softmax comes from the float32 row statistics.  The same bits on every run: the posteriors of the label
 * positions that name one token are summed as 64-bit integers in units of 2^-40, Gamma_t and the blank's share lane-wise in a fixed
 * order; no floating-point atomics anywhere.
 * Workspace (may hold anything on entry).  want_grad == 0 (grad == NULL): 0 bytes, the pointer may be NULL.  Otherwise, with S = 2
 * (classic) or 1 (simplified), NL the smallest power of two with 64 * NL >= U (1 for U <= 64) and r256(x) = x rounded up to a
 * multiple of 256:
 *   ctc_amd_wildcard_loss_workspace_bytes = r256(8 * B * T * (S * 64 * NL + 2)) + r256(16 * B * T) + r256(8 * B)
 * -- the chain's float64 state of every frame (overwritten by the posteriors), the row statistics, log2 Z.  B = 256, T = 1000,
 * U = 128: 532.5 MB classic, 270.3 MB simplified (section 7 names what would cut it).  A call with
 * grad == NULL accepts any workspace; one with grad != NULL needs the want_grad size.
 * One launch of B workgroups without a gradient; with one, the alpha sweep that keeps its rows, the beta sweep (B workgroups each)
 * and one wavefront per row (b, t) (T == 0: the first alone).  No allocation, copy or synchronisation; asynchronous on `stream`,
 * capturable.
 */
int ctc_amd_wildcard_loss_workspace_bytes(int kind, int B, int T, int V, int U, int want_grad, size_t *out_bytes /*host*/);
int ctc_amd_wildcard_loss_grad(int kind, int wrt,
                               const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                               const int32_t *labels, int label_stride,
                               const int32_t *label_length, const int32_t *logit_length, int blank_index,
                               float wildcard_log_weight, int B, int T, int V, int U,
                               const float *d_loss /* [B], NULL = ones */, float *loss /* [B] */,
                               void *grad /* NULL = forward only */, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * Long-form CTC loss and gradient: ctc_amd_wildcard_loss_grad for U <= CTC_AMD_LONG_MAX_U label positions (added under ABI v6: two
 * new entry points, nothing existing changed).  The confidence -ln P(transcript | recording) of a recording aligned with
 * ctc_amd_long_wildcard_best_path, and training on it without cutting it up.
 *
 * Labels, lengths, blank, formats, lattices, emissions, wildcard_log_weight, the loss, the gradient with respect to logits or
 * log-probabilities, d_loss, infeasible utterances (loss +inf, an exactly zero gradient, d_loss[b] not interpreted), every degenerate
 * case and what is written (every gradient row t < T of every utterance, nothing between V and a larger stride) are those of
 * ctc_amd_wildcard_loss_grad; a transcript without CTC_AMD_WILDCARD is the plain CTC loss.  First derivatives only.
 * The lattice is tiled as in ctc_amd_long_best_path: K = max(1, ceil(U / 1024)) label blocks x J = max(1, ceil(T / TF)) time blocks
 * of TF = frames_per_tile frames (0: CTC_AMD_LONG_FRAMES_DEFAULT; otherwise a positive multiple of CTC_AMD_LONG_FRAMES_MULTIPLE).
 * The alpha sweep runs one launch per anti-diagonal of tiles (K + J - 1), a finish kernel takes log2 Z; with a gradient the beta
 * sweep runs the anti-diagonals in reverse and one wavefront per row (b, t) writes the gradient.  The order of the launches on the
 * stream is the only dependency: no workgroup waits for another.  Tiles wholly beyond an utterance's frames or labels, or wholly
 * before the first frame their positions can be reached in, do not run.
 * Numerics: those of ctc_amd_wildcard_loss_grad (float64 base-2 logarithms with a true -inf in both sweeps and in everything handed
 * from tile to tile, float32 row statistics taken once per frame, integer sums of the posteriors).  The same bits on every run, for
 * every frames_per_tile and for every batch composition; no floating-point atomics.
 * Validation follows ctc_amd_wildcard_loss_grad in its order and with its messages: common arguments (U <= CTC_AMD_LONG_MAX_U in
 * place of CTC_AMD_MAX_U), element types, B == 0 (CTC_AMD_OK without a launch), strides (the gradient's only when grad != NULL),
 * wildcard_log_weight, loss non-NULL, V <= CTC_AMD_MAX_V, B * T < 2^33 when grad != NULL; then frames_per_tile and the tile grid
 * (B * min(K, J) <= 2^31 - 1 workgroups) as in ctc_amd_long_best_path (CTC_AMD_EINVAL each); then the workspace
 * (CTC_AMD_EWORKSPACE before any launch).
 * Workspace (may hold anything on entry; needed without a gradient too), every term a size_t, r256(x) = x rounded up to a multiple
 * of 256, S = 2 (classic) or 1 (simplified):
 *   ctc_amd_long_wildcard_loss_workspace_bytes =
 *       r256(16 * B * (K - 1) * T)          alpha columns: the pair (O, C) of a block's last position before every frame, float64
 *     + r256(8 * B * K * 2056)              alpha row buffers: the chain state between the time blocks of a label block, float64
 *     + r256(16 * B * T)                    row statistics of every frame: x[blank], max, log2 sum exp, float32
 *     + r256(8 * B)                         log2 Z, float64
 *     + r256(4 * B)                         feasible, int32
 *   and, with want_grad != 0 (grad != NULL),
 *     + r256(8 * B * (K - 1) * T)           beta columns: the worth of entering a block's first position with every frame, float64
 *     + r256(8 * B * K * 2056)              beta row buffers
 *     + r256(8 * B * K * T * (S * 1024 + 2))  the chain's float64 state of every frame and label block (overwritten by the posteriors)
 * The last term is all that matters: B = 1, T = 30 000, U = 8 192 takes 3 941 783 808 bytes classic and 1 975 703 808 simplified with
 * a gradient and 3 972 096 without one; an hour of audio (T = 180 000, U = 50 000) 144.9 GB with a gradient, which fits no card, and
 * 141.9 MB without one (section 7 names what would cut it).  A call with grad == NULL accepts the want_grad
 * size too.  No allocation, copy or synchronisation; asynchronous on `stream`, capturable; the number of launches depends on T, U
 * and frames_per_tile alone.
 */
int ctc_amd_long_wildcard_loss_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, int want_grad,
                                               size_t *out_bytes /*host*/);
int ctc_amd_long_wildcard_loss_grad(int kind, int wrt,
                                    const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                    const int32_t *labels, int label_stride,
                                    const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                    float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                    const float *d_loss /* [B], NULL = ones */, float *loss /* [B] */,
                                    void *grad /* NULL = forward only */, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t,
                                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Long-form CTC loss and gradient from tile checkpoints: ctc_amd_long_wildcard_loss_grad with a workspace that keeps no per-frame
 * chain rows for the whole recording, so that an hour of audio fits one card with its gradient (added under ABI v6: two new entry
 * points, nothing existing changed).
 *
 * Contract: every word of ctc_amd_long_wildcard_loss_grad's -- arguments, lattices, formats, degenerate cases, what is written --
 * and the same bits in loss and gradient for the same inputs and any frames_per_tile: the chain step, the posteriors and the row
 * stage are the same code, and what a tile starts from is the same float64 state.  With grad == NULL the call IS
 * ctc_amd_long_wildcard_loss_grad (same launches, same workspace size).
 * Schedule, with K, J, TF as there and R = min(K, J):
 *   forward   the alpha tiles on the K + J - 1 anti-diagonals, keeping no per-frame rows; the chain row that leaves tile (k, j) goes
 *             to a checkpoint of its own, [b][k][j], and tile (k, j + 1) starts from it.  The finish kernel takes log2 Z from the
 *             checkpoint of the last tile in time of block (L - 1) / 1024.  K + J launches.
 *   backward  per reverse anti-diagonal d = K + J - 2 .. 0: the alpha tiles (k, d - k) run again from their checkpoints (and the
 *             alpha columns and row statistics the forward sweep left) and save their per-frame rows into slot j mod R of a ring
 *             per (utterance, label block); the beta tiles of the diagonal turn those rows into posteriors, as in the existing
 *             call; then, tile (0, d) having been the last of time block d, the row stage writes the gradient rows of frames
 *             d * TF .. min(T, d * TF + TF) - 1 of every utterance (d < J).  2 (K + J - 1) + J launches.
 *   The time blocks in flight on diagonal d are d - K + 1 .. d, K consecutive ones, so distinct modulo R; slot (d - R) mod R is next
 *   written on diagonal d - 1, behind the row stage of time block d on the stream.  J < K: every time block has a slot of its own.
 *   Every gradient row (b, t) is written exactly once.  The order of the launches on the stream is the only dependency.
 * Validation: that of ctc_amd_long_wildcard_loss_grad, in its order and with its messages (B * T < 2^33 with a gradient included:
 * it is not relaxed, although the row stage's grids are B * TF rows here).
 * Workspace (may hold anything on entry), in the terms of ctc_amd_long_wildcard_loss_workspace_bytes.  want_grad == 0: that
 * function's value.  want_grad != 0:
 *   ctc_amd_long_wildcard_loss_ckpt_workspace_bytes =
 *       r256(16 * B * (K - 1) * T)                 alpha columns                        (as there)
 *     + r256(8 * B * K * J * 2056)                 alpha checkpoints                    (there: 8 * B * K * 2056)
 *     + r256(16 * B * T) + r256(8 * B) + r256(4 * B)   row statistics, log2 Z, feasible (as there)
 *     + r256(8 * B * (K - 1) * T)                  beta columns                         (as there)
 *     + r256(8 * B * K * 2056)                     beta row buffers                     (as there)
 *     + r256(8 * B * K * min(R * TF, T) * (S * 1024 + 2))   the ring of saved rows      (there: 8 * B * K * T * (S * 1024 + 2))
 *   (J = max(1, ceil(T / TF)) as above.  min(R * TF, T): with R = J the last time block is short and the slots are the T per-frame
 *   rows themselves, so the ring never exceeds the term it replaces; T = 0: no rows.)
 * B = 1, T = 30 000, U = 8 192: 170 923 264 bytes classic (3 941 783 808 there, 23 x), 103 814 400 simplified.  An hour of audio
 * (T = 180 000, U = 50 000; K = 49, J = 1407): 6 385 200 384 bytes classic, 3 867 569 408 simplified, against 144.9 / 72.6 GB.
 * frames_per_tile trades memory here: the ring grows with TF, the checkpoints with 1 / TF (the hour at TF = 32: 6.0 GB, at TF = 512:
 * 20.7 GB).  The price is one more alpha sweep.  No allocation, copy or synchronisation; asynchronous on
 * `stream`, capturable; the number of launches depends on T, U and frames_per_tile alone.
 */
int ctc_amd_long_wildcard_loss_ckpt_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, int want_grad,
                                                    size_t *out_bytes /*host*/);
int ctc_amd_long_wildcard_loss_grad_ckpt(int kind, int wrt,
                                         const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                         const int32_t *labels, int label_stride,
                                         const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                         float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                         const float *d_loss /* [B], NULL = ones */, float *loss /* [B] */,
                                         void *grad /* NULL = forward only */, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t,
                                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * Label posteriors: the soft alignment of a transcript over all CTC paths (added under ABI v6: two new entry points, nothing
 * existing changed).  What a forward-backward pass says most directly: with what probability frame t belongs to label position i,
 * over all alignments -- per POSITION, not per token, so repeated labels and wildcards keep their own columns.  Forward only.
 *
 * Inputs, lattices, emissions, wildcard_log_weight, infeasible utterances, formats and strides are exactly those of
 * ctc_amd_wildcard_loss_grad (a transcript without CTC_AMD_WILDCARD is the plain CTC lattice).  L = label_length[b], T_b =
 * logit_length[b] clamped to [0, T].  The posterior of a state (classic) or of a step (simplified) at frame t is the share of Z that
 * passes through it.  For a feasible utterance, t < T_b and i < L:
 * Classic lattice.
 *   label_posterior[b, t, i] = the posterior of the open state of position i after frame t (the state that emits label i, or e_w
 *                              for a wildcard);
 *   blank_posterior[b, t]    = the sum of the posteriors of all closed states and of the start state (all of which emit the blank).
 * Simplified lattice.
 *   label_posterior[b, t, i] = the posterior of entering position i at frame t; if position i is a wildcard, plus the posterior of
 *                              staying in the state behind it at frame t (which emits e_w);
 *   blank_posterior[b, t]    = the sum of the posteriors of all stays that emit the blank (behind an ordinary label, and in the
 *                              start state).
 * Both: sum_i label_posterior[b, t, i] + blank_posterior[b, t] = 1.
 *   duration[b, i]       = sum_t label_posterior[b, t, i]: the expected number of frames of position i;
 *   expected_frame[b, i] = sum_t t * label_posterior[b, t, i] / duration[b, i]: the soft timestamp.
 * duration and expected_frame ARE DEFINED AS REDUCTIONS OF THE FLOAT32 label_posterior VALUES THE CALL RETURNS: both sums run in
 * float64 over t < T_b in a fixed order (eight contiguous runs of frames, each in frame order, then the runs in frame order), the
 * quotient is taken in float64 of the two unrounded sums, and each result is rounded once to float32.  A float64 host reduction of
 * the returned matrix therefore reproduces them to the last float32 bit or two.
 *   loss[b] = -ln Z[b]: the same bits as ctc_amd_wildcard_loss_grad returns forward-only on the same arguments.
 * Every element of every output is written, so the caller never has to clear a buffer: frames t >= T_b get 0 in label_posterior and
 * blank_posterior; positions L <= i < U get 0 in label_posterior and duration and -1 in expected_frame; an infeasible utterance gets
 * loss +inf, zeros, and -1 in expected_frame, and changes nothing else in the batch.
 * On every path each position holds at least one frame, so duration >= 1 for i < L of a feasible utterance (up to the rounding of
 * the posteriors); it is 1 for an ordinary label on the simplified lattice, which is entered exactly once.  label_length == 0: the
 * all-blank path, blank_posterior = 1 for t < T_b.  T_b == 0: loss 0 for an empty transcript, +inf otherwise; nothing to write for
 * t.  NaN and +inf inputs: unspecified, the call completes.
 *   loss[B], label_posterior[B][T][U], blank_posterior[B][T] float32, contiguous; duration[B][U], expected_frame[B][U] float32,
 *   both given or both NULL (then no statistics work is done and the other outputs are the same bits).
 * Validation in the order of ctc_amd_wildcard_loss_grad: common arguments, element type, B == 0 (CTC_AMD_OK without a launch),
 * strides, wildcard_log_weight; then loss non-NULL, label_posterior non-NULL when T > 0 and U > 0, blank_posterior non-NULL when
 * T > 0, duration and expected_frame both or neither; V <= CTC_AMD_MAX_V (U <= CTC_AMD_MAX_U is a common argument; no launch grid
 * here depends on B * T) (CTC_AMD_EINVAL each); then the workspace (CTC_AMD_EWORKSPACE before any launch).
 * Numerics: the sweeps of ctc_amd_wildcard_loss_grad -- the alpha sweep is its gradient path's, bit for bit; a posterior is the
 * float32 exp2 of a float64 difference; blank_posterior is summed over the wavefront in a fixed order.  Every element has one
 * writer, there are no atomics: the same bits on every run.
 * Workspace (may hold anything on entry): that of ctc_amd_wildcard_loss_grad with a gradient,
 *   ctc_amd_label_posterior_workspace_bytes = ctc_amd_wildcard_loss_workspace_bytes(want_grad = 1)
 *                                           = r256(8 * B * T * (S * 64 * NL + 2)) + r256(16 * B * T) + r256(8 * B)
 * (section 7 names what would cut it).  Launches: the alpha sweep, the beta sweep (B workgroups each; T == 0:
 * the first alone) and, when duration is given and U > 0, one launch of a workgroup per utterance and 64 positions.  No allocation, copy or
 * synchronisation; asynchronous on `stream`, capturable.
 */
int ctc_amd_label_posterior_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes /*host*/);
int ctc_amd_label_posterior(int kind, int wrt,
                            const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                            const int32_t *labels, int label_stride,
                            const int32_t *label_length, const int32_t *logit_length, int blank_index,
                            float wildcard_log_weight, int B, int T, int V, int U,
                            float *loss /* [B] */, float *label_posterior /* [B][T][U] */, float *blank_posterior /* [B][T] */,
                            float *duration /* [B][U], may be NULL */, float *expected_frame /* [B][U], may be NULL */,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * Long-form label posteriors: ctc_amd_label_posterior for U <= CTC_AMD_LONG_MAX_U label positions, and a per-label confidence that
 * needs no [B][T][U] matrix (added under ABI v6: two new entry points, nothing existing changed).  Which stretches of a ten-minute
 * or one-hour alignment to trust: the best path of ctc_amd_long_wildcard_best_path cannot say, the posteriors can.
 *
 * Inputs, lattices, emissions, wildcard_log_weight, infeasible utterances, formats (float32 / bfloat16 / float16) and strides
 * (logits read in place) are those of ctc_amd_long_wildcard_loss_grad; the meaning of label_posterior, blank_posterior, duration
 * and expected_frame is that of ctc_amd_label_posterior.  Forward only.  L = label_length[b], T_b = logit_length[b] clamped to
 * [0, T].  The outputs, all contiguous:
 *   loss[B]                  the bits of ctc_amd_long_wildcard_loss_grad.
 *   label_posterior[B][T][U] MAY BE NULL (T = 180 000, U = 50 000 would be 36 GB): then it is not written and every other output
 *                            keeps its bits.  Otherwise, for t < T_b and i < L of a feasible utterance, the float32 posterior the
 *                            beta sweep forms -- classic: of the open state of position i after frame t; simplified: of entering
 *                            position i at frame t, plus (added in float32) that of staying behind it when it is a wildcard -- the
 *                            values ctc_amd_label_posterior returns; exactly 0 in a tile that does not run (wholly before the
 *                            first frame its positions can be reached in).
 *   blank_posterior[B][T]    the closed states' (classic) or the blank-emitting stays' (simplified) posteriors plus the start
 *                            state's, summed in float32 in one fixed order that depends on neither frames_per_tile nor the batch:
 *                            lane l of a wavefront takes positions l, l + 64, ... of label block 0, then of block 1, and so on
 *                            (lane 0 the start state behind block 0), then the 64 lanes are summed.
 *   duration[B][U], expected_frame[B][U]   both or neither.  REDUCTIONS OF THE FLOAT32 label_posterior VALUES (returned or not):
 *                            sum_t p and sum_t t * p run in float64, STRICTLY SEQUENTIALLY IN DESCENDING FRAME ORDER, from T_b - 1
 *                            to 0 (the backward sweep meets the time blocks in that order, and a sequential sum carried from block
 *                            to block is the same sequence whatever frames_per_tile is; t * p is exact in float64); the quotient
 *                            is taken in float64 and each result is rounded once.  A float64 host reduction of the returned matrix
 *                            in that order reproduces them bit for bit.
 *   peak_posterior[B][U] float32, peak_frame[B][U] int32   both or neither.  max_t label_posterior[b, t, i] and the lowest t that
 *                            attains it: the per-label confidence when the dense matrix does not fit.
 * Every element of every given output is written: frames t >= T_b get 0 in label_posterior and blank_posterior; positions
 * L <= i < U get 0 in label_posterior, duration and peak_posterior and -1 in expected_frame and peak_frame; an infeasible utterance
 * gets loss +inf, zeros and -1 and changes nothing else in the batch.  T == 0 still writes the [B][U] outputs (0 / -1).
 * Schedule: that of ctc_amd_long_wildcard_loss_grad_ckpt, with a posterior stage in the row stage's place: after the beta tiles of
 * reverse anti-diagonal d < J one launch reads the ring rows of time block d -- a wavefront per row (b, t) writes the dense run and
 * blank_posterior[b, t]; a wavefront per (b, 64 positions) walks the block's frames downwards and carries sum p, sum t p, the peak
 * and its frame in the workspace (the stage of block J - 1 starts them, that of block 0 rounds and writes).  No workgroup waits for
 * another; vector stores only, one writer per element, no atomics: the same bits on every run, for every frames_per_tile and every
 * batch composition.  K + J launches forward and 2 (K + J - 1) + J backward, as there (T == 0: 1 or 2).
 * Validation: that of ctc_amd_long_wildcard_loss_grad_ckpt with a gradient, in its order and with its messages -- common arguments
 * (U <= CTC_AMD_LONG_MAX_U), element type, B == 0 (CTC_AMD_OK without a launch), strides, wildcard_log_weight, loss non-NULL,
 * V <= CTC_AMD_MAX_V, B * T < 2^33 --; then blank_posterior non-NULL when T > 0, duration / expected_frame both or neither,
 * peak_posterior / peak_frame both or neither; then frames_per_tile and the launch grids (CTC_AMD_EINVAL each); then the workspace
 * (CTC_AMD_EWORKSPACE before any launch).
 * Workspace (may hold anything on entry):
 *   ctc_amd_long_label_posterior_workspace_bytes = ctc_amd_long_wildcard_loss_ckpt_workspace_bytes(want_grad = 1)
 *     + r256(16 * B * U)                    sum p and sum t p of every position, float64
 *     + r256(8 * B * U)                     the running peak (float32) and its frame (int32)
 * B = 1, T = 30 000, U = 8 192: 171 119 872 bytes classic; the hour (T = 180 000, U = 50 000): 6 386 400 512 classic.  No
 * allocation, copy or synchronisation; asynchronous on `stream`, capturable; the number of launches depends on T, U and
 * frames_per_tile alone.
 */
int ctc_amd_long_label_posterior_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, size_t *out_bytes /*host*/);
int ctc_amd_long_label_posterior(int kind, int wrt,
                                 const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                 const int32_t *labels, int label_stride,
                                 const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                 float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                 float *loss /* [B] */, float *label_posterior /* [B][T][U], may be NULL */,
                                 float *blank_posterior /* [B][T] */,
                                 float *duration /* [B][U], may be NULL */, float *expected_frame /* [B][U], may be NULL */,
                                 float *peak_posterior /* [B][U], may be NULL */, int32_t *peak_frame /* [B][U], may be NULL */,
                                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * Edit counts (added under ABI v6: two new entry points, nothing existing changed): what an error-rate report prints -- distance,
 * substitutions, insertions, deletions -- of every hypothesis against its utterance's reference, for references of up to
 * CTC_AMD_LONG_MAX_U tokens.  ctc_amd_edit_distance keeps its limit of CTC_AMD_MAX_U and its single number.
 * Rows of the table are hypothesis tokens (i = 0 .. h), columns reference tokens (j = 0 .. r).  A move up, (i - 1, j) -> (i, j), is
 * an insertion (a hypothesis token with no reference token); a move left, (i, j - 1) -> (i, j), a deletion; a diagonal move a hit
 * if the two tokens are equal and a substitution otherwise.  Every cell carries the triple (d, S, I) -- distance, substitutions,
 * insertions --, a move adds (1, 0, 1), (1, 0, 0), (0, 0, 0) or (1, 1, 0), and a cell keeps the LEXICOGRAPHIC MINIMUM of its three
 * candidates; the boundaries are (j, 0, 0) in row 0 and (i, 0, i) in column 0.  Addition is monotone in that order, so the result is
 * the lexicographic minimum of (d, S, I) over all alignments: among the alignments of minimum distance the one with the fewest
 * substitutions (the most hits), then the fewest insertions.  It names no path, so it depends on no tie rule of a back-trace.
 *   counts[b, n] = (d, S, I, d - S - I)                                          int32 [B][N][4], exact
 *   hits = h - S - I = r - S - deletions.   hyp (0, 1) against ref (1, 0): (2, 0, 1, 1), one hit.
 * Layouts, length clamping and token semantics are those of ctc_amd_edit_distance: tokens at and beyond the lengths are not read;
 * h == 0 gives (r, 0, 0, r) and r == 0 gives (h, 0, h, 0).
 * R bounds every reference length, 0 <= R <= CTC_AMD_LONG_MAX_U: an utterance with r > R gets -1 four times for all its hypotheses
 * and changes nothing else.  0 <= hyp_stride <= CTC_AMD_EDIT_COUNTS_MAX_STRIDE.  rows_per_tile is 0 (the default, 256) or a
 * positive multiple of CTC_AMD_EDIT_COUNTS_ROWS_MULTIPLE: a tile of the table is 1024 reference tokens x rows_per_tile hypothesis
 * tokens, and the result does not depend on it.  N >= 1, B * N < 2^31, and no launch grid beyond 2^31 - 1 workgroups
 * (B * N * min(K, J) / 4).  B == 0 returns CTC_AMD_OK without a launch.
 * Validation before any launch (CTC_AMD_EINVAL, ctc_amd_last_error), in the order of ctc_amd_edit_distance: negative B or R, R
 * beyond its limit, N < 1, the product limit, negative strides, hyp_stride beyond its limit, rows_per_tile, the launch grid, null
 * lengths, null hyp / ref (allowed when their stride is 0), null counts; then a null or too small workspace (CTC_AMD_EWORKSPACE).
 * Every element of `counts` has one writer; counts[b, n] is the same whatever N, rows_per_tile and the other hypotheses are, wherever
 * in the list it stands, and on every run.
 * Workspace (8-byte aligned; may hold anything on entry), with K = max(1, ceil(R / 1024)):
 *   ctc_amd_edit_counts_workspace_bytes = r256(8 * B * N * (K - 1) * hyp_stride)   the last column of every column block but the last
 *                                       + r256(8 * B * N * K * 1024)               the bottom row of the tile above, per column block
 * in packed words d * 2^42 + S * 2^21 + I, r256 rounding up to a multiple of 256.  B = 1, N = 1, R = hyp_stride = 65 536: 33 554 432
 * bytes.
 * K + J - 1 launches, J = max(1, ceil(hyp_stride / rows_per_tile)): one per anti-diagonal of tiles, one wavefront per tile, tiles
 * wholly beyond a pair's own (h, r) return at once; R <= 512 runs one column block with 1, 2, 4 or 8 reference tokens per lane in
 * place of 16.  Asynchronous on `stream`, capturable (a serial chain of launches), no allocation, copy or synchronisation; the
 * number of launches depends on R, hyp_stride and rows_per_tile alone.
 */
#define CTC_AMD_EDIT_COUNTS_MAX_STRIDE 1048576  /* 2^20: d, S, I each fit 21 bits */
#define CTC_AMD_EDIT_COUNTS_ROWS_MULTIPLE 64
int ctc_amd_edit_counts_workspace_bytes(int B, int N, int R, int hyp_stride, int rows_per_tile, size_t *out_bytes /*host*/);
int ctc_amd_edit_counts(const int32_t *hyp, int hyp_stride, const int32_t *hyp_length /* [B][N] */,
                        const int32_t *ref, int ref_stride, const int32_t *ref_length /* [B] */,
                        int B, int N, int R, int rows_per_tile /* 0: default */,
                        int32_t *counts /* [B][N][4]: distance, substitutions, insertions, deletions */,
                        void *workspace, size_t workspace_bytes, void *stream);

/*
 * Frame windows per label: time-constrained CTC loss, posteriors and forced alignment (added under ABI v6: four new entry points,
 * then the three long-form ones of the loss, its checkpointed twin and the label posteriors; nothing existing changed).  A caller who knows roughly where every label belongs -- a reference alignment and a tolerance
 * (alignment-restricted training), subtitles or a coarse first pass, another model's first_frame / last_frame or expected_frame --
 * says so per label POSITION.  A mask on the logits cannot: it is per token, and the same token at two positions needs two masks.
 *
 * Each entry point is its counterpart with two more arguments behind blank_index, and is otherwise its counterpart in every
 * respect: inputs, formats, strides, outputs, limits, validation order and messages, workspace (the counterpart's size query; a
 * window needs none), launches, capture.
 *   ctc_amd_windowed_loss_grad         ctc_amd_wildcard_loss_grad        (the loss alone, or the loss and its gradient)
 *   ctc_amd_windowed_label_posterior   ctc_amd_label_posterior
 *   ctc_amd_windowed_best_path         ctc_amd_wildcard_best_path
 *   ctc_amd_long_windowed_best_path    ctc_amd_long_wildcard_best_path   (U <= CTC_AMD_LONG_MAX_U)
 *   ctc_amd_long_windowed_loss_grad        ctc_amd_long_wildcard_loss_grad        (U <= CTC_AMD_LONG_MAX_U; the loss alone, or with
 *                                                                                  its gradient from the per-frame workspace)
 *   ctc_amd_long_windowed_loss_grad_ckpt   ctc_amd_long_wildcard_loss_grad_ckpt   (the same bits from tile checkpoints)
 *   ctc_amd_long_windowed_label_posterior  ctc_amd_long_label_posterior           (label_posterior may be NULL, as there)
 *   frame_window   int32 [B][window_stride] device memory: (first, last) = frame_window[b * window_stride + 2 i], [.. + 2 i + 1]
 *                  for label position i, BOTH INCLUSIVE -- the convention of the first_frame / last_frame outputs, which can be
 *                  fed back in.  NULL: the unwindowed call, bit for bit, whatever window_stride holds.
 *   window_stride  int32 elements between utterances, >= 2 * U when frame_window is given (CTC_AMD_EINVAL otherwise; checked
 *                  behind the counterpart's own argument checks and before the workspace).
 * Position i of utterance b may OWN frame t only if first <= t <= last.  To own a frame is what the alignment calls report as
 * label_index[b, t] == i:
 *   classic lattice     the frames spent in the open state of position i (for a wildcard: its open state, which emits m_t / e_w);
 *   simplified lattice  the frame of the diagonal step into position i; for a wildcard also every frame of a horizontal step
 *                       behind it, for which it pays m_t / e_w.
 * Frames that emit the blank are never constrained (closed states and the start state; simplified: horizontal steps behind an
 * ordinary label and in the start state).  A wildcard position obeys its window like any other.
 * Outside its window the emission of a position is -inf.  The summed lattice (loss, gradient, posteriors) and the maximised one
 * (alignment) are otherwise those of the counterparts, with their tie rules: the recursions read
 *     e[i](t) = -inf when t < first_i or t > last_i, else the counterpart's e[i](t)
 * in every place where position i emits, the horizontal m_t / e_w of a simplified wildcard included.
 *   - The values are read on the device only and are not validated: first < 0 and last >= T_b act as clipped to [0, T_b - 1].
 *   - first > last is an empty window: the position cannot emit, so the utterance is infeasible exactly as the counterpart's
 *     infeasible utterances are -- loss +inf, a zero gradient, zero posteriors, score -inf and the documented degenerate outputs --
 *     and changes nothing else in the batch.  So is every utterance whose windows admit no path.
 *   - Positions at or beyond label_length[b] are ignored (their pairs may hold anything, but the memory must be there).
 *   - label_posterior is exactly 0 outside a position's window; every frame's posteriors still sum to 1.
 * Windows that cover every frame return the bits of the unwindowed call for every output.  Long-form: frames are absolute; no
 * output depends on where a window's edges fall relative to time blocks or label blocks, on frames_per_tile or on the batch, as for
 * the counterpart.  Tiles that no window reaches still run.  That holds for the three long-form calls of the
 * summed lattice as for the alignment: the pair of position i is frame_window[b * window_stride + 2 i], [.. + 2 i + 1] for every
 * i < label_length[b] <= CTC_AMD_LONG_MAX_U, whichever label block i falls into; ctc_amd_long_windowed_loss_grad_ckpt returns the
 * bits of ctc_amd_long_windowed_loss_grad and the loss of ctc_amd_long_windowed_label_posterior is theirs; an hour aligned with
 * ctc_amd_long_windowed_best_path (or unconstrained) and widened by a tolerance is a valid window for all three (DESIGN.md
 * section 5.25).
 * Numerics, determinism and cost are the counterparts': the producers compare the frame with the two bounds as they gather the
 * emissions, one block ahead of the chain.
 */
int ctc_amd_windowed_loss_grad(int kind, int wrt,
                               const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                               const int32_t *labels, int label_stride,
                               const int32_t *label_length, const int32_t *logit_length, int blank_index,
                               const int32_t *frame_window /* [B][window_stride], may be NULL */, int window_stride,
                               float wildcard_log_weight, int B, int T, int V, int U,
                               const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                               int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_windowed_label_posterior(int kind, int wrt,
                                     const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                     const int32_t *labels, int label_stride,
                                     const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                     const int32_t *frame_window /* [B][window_stride], may be NULL */, int window_stride,
                                     float wildcard_log_weight, int B, int T, int V, int U,
                                     float *loss, float *label_posterior, float *blank_posterior, float *duration,
                                     float *expected_frame, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_windowed_best_path(int kind, int wrt,
                               const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                               const int32_t *labels, int label_stride,
                               const int32_t *label_length, const int32_t *logit_length, int blank_index,
                               const int32_t *frame_window /* [B][window_stride], may be NULL */, int window_stride,
                               int B, int T, int V, int U,
                               float *score, int32_t *tokens, int32_t *label_index, int32_t *first_frame, int32_t *last_frame,
                               float *label_score, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_long_windowed_best_path(int kind, int wrt,
                                    const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                    const int32_t *labels, int label_stride,
                                    const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                    const int32_t *frame_window /* [B][window_stride], may be NULL */, int window_stride,
                                    int B, int T, int V, int U, int frames_per_tile,
                                    float *score, int32_t *tokens, int32_t *label_index, int32_t *first_frame, int32_t *last_frame,
                                    float *label_score, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_long_windowed_loss_grad(int kind, int wrt,
                                    const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                    const int32_t *labels, int label_stride,
                                    const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                    const int32_t *frame_window /* [B][window_stride], may be NULL */, int window_stride,
                                    float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                    const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                                    int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_long_windowed_loss_grad_ckpt(int kind, int wrt,
                                         const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                         const int32_t *labels, int label_stride,
                                         const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                         const int32_t *frame_window /* [B][window_stride], may be NULL */, int window_stride,
                                         float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                         const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                                         int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_long_windowed_label_posterior(int kind, int wrt,
                                          const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                          const int32_t *labels, int label_stride,
                                          const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                          const int32_t *frame_window /* [B][window_stride], may be NULL */, int window_stride,
                                          float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                          float *loss, float *label_posterior, float *blank_posterior, float *duration,
                                          float *expected_frame, float *peak_posterior, int32_t *peak_frame,
                                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Optional wildcards: a wildcard position that may be empty (added under ABI v6: two new entry points with their size queries,
 * nothing existing changed).  CTC_AMD_WILDCARD stands for a NON-EMPTY run of frames.  Star temporal classification puts a star
 * between every pair of labels and lets each be empty; a lightly supervised transcript says that something MAY be missing
 * between two words; a keyword may or may not be preceded by filler.  For those there is a second reserved label value,
 * CTC_AMD_OPTIONAL_WILDCARD = -3, accepted by
 *   ctc_amd_optional_wildcard_loss_grad         counterpart: ctc_amd_wildcard_loss_grad   (the loss alone, or with its gradient)
 *   ctc_amd_optional_wildcard_label_posterior   counterpart: ctc_amd_label_posterior
 *   ctc_amd_optional_wildcard_best_path         counterpart: ctc_amd_wildcard_best_path
 * only.  Each is its counterpart in arguments, formats, strides, outputs, limits (U <= CTC_AMD_MAX_U), validation order and
 * messages, workspace (the size queries return the counterparts' sizes), launches and capture.  In every other entry point -3
 * stays what it was: a label outside [0, V), an infeasible utterance.  ctc_amd_check_labels keeps rejecting both values.
 * One limit differs: ctc_amd_optional_wildcard_best_path on the CLASSIC lattice takes U <= CTC_AMD_OPTIONAL_CLASSIC_MAX_U = 512
 * (CTC_AMD_EINVAL beyond, behind the counterpart's argument checks and before the workspace; the size query says so too): the
 * chain step for 16 positions per lane does not fit the register file without scratch, and no spilling kernel is shipped.  The
 * simplified alignment, the loss and the posteriors take U <= CTC_AMD_MAX_U.
 * The long-form loss, gradient and label posteriors take it too (below); there is no long-form alignment, N-best or frame-window
 * variant.
 *
 * Let position i be an optional wildcard.  Everything said of a wildcard holds for it when it is used: the emission e_w(t),
 * contiguous frames, its own posterior column.  In addition it may be skipped:
 * Classic lattice.  Skipping i adds two sources to the open state of i + 1:
 *   - the closed state of i - 1, or the start state when i = 0;
 *   - the open state of i - 1, when label[i + 1] != label[i - 1] or either is a wildcard of either kind.
 * The closed state of i is reachable only through i's open state, so a path that skips i waits in the closed state of i - 1 and
 * no path is counted twice.  If i is the last position, the open and closed states of i - 1 are end states too; for
 * label_length = 1 that is the start state.
 * Simplified lattice.  State i + 1 may also be entered from state i - 1 (the start state when i = 0), at the cost of label
 * i + 1's emission.  If i is last, state i - 1 is an end state too.
 * Equivalence.  The set of state sequences is the disjoint union, over all subsets of the optional positions, of the state
 * sequences of the transcript with that subset deleted and the remaining optional wildcards made mandatory.  Hence Z is the sum
 * of those transcripts' Z, and gradients and posteriors are the Z-weighted mixtures, posterior columns mapped back to the
 * original positions with zero columns for the skipped ones.
 * Adjacency.  Two optional wildcards may not be adjacent (a chain of skips would need unbounded reach): such an utterance is
 * infeasible, like a bad label.  An optional wildcard next to a mandatory one is allowed.
 * Best path.  It is the best over those transcripts.  emission m_t, tokens = a_t where the position is used.  Ties: the candidates
 * of a position's open state stay in the order stay, closed i - 1, open i - 1, closed i - 2, open i - 2 (simplified: stay, i - 1,
 * i - 2) with strict comparisons, the end states in the order closed, open of L - 1, closed, open of L - 2: deterministic, the same
 * bits on every run.  Outputs for a skipped position: first_frame = last_frame = -1 and label_score = 0.0, the log-probability of
 * an empty run, so that sum_i label_score + the blank frames still equals score.  Back-pointers: the counterpart's words and
 * workspace size -- classic, source code 3 of a position's 3 bits and the word's one spare bit per position; simplified, a second
 * bit per position.  A transcript without an optional wildcard returns the counterpart's bits for every output.
 * Posteriors.  The column of an optional wildcard may sum to less than 1 frame: duration >= 0 there, expected_frame = -1 where
 * duration is 0.  A frame's values still sum to 1.
 * Short utterances.  The frames an utterance needs no longer count optional wildcards.  T_b = 0 is feasible, with loss 0, for
 * label_length = 0 or for a single optional wildcard.
 * A transcript without an optional wildcard returns the bits of the counterpart for every output.  Numerics and determinism
 * are the counterparts'; the chain step has two more terms per position.
 * d_loss[b] == 0: the gradient of utterance b is +0 in every element, as for an infeasible utterance (the counterparts return
 * 0 * g, which is -0 where g is negative); the long-form entry points below do the same.
 */
#define CTC_AMD_OPTIONAL_WILDCARD (-3)
#define CTC_AMD_OPTIONAL_CLASSIC_MAX_U 512
int ctc_amd_optional_wildcard_best_path_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes /*host*/);
int ctc_amd_optional_wildcard_best_path(int kind, int wrt,
                                        const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                        const int32_t *labels, int label_stride,
                                        const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                        int B, int T, int V, int U,
                                        float *score, int32_t *tokens, int32_t *label_index /* may be NULL */,
                                        int32_t *first_frame /* may be NULL */, int32_t *last_frame /* may be NULL */,
                                        float *label_score /* may be NULL */, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_optional_wildcard_loss_workspace_bytes(int kind, int B, int T, int V, int U, int want_grad, size_t *out_bytes /*host*/);
int ctc_amd_optional_wildcard_loss_grad(int kind, int wrt,
                                        const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                        const int32_t *labels, int label_stride,
                                        const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                        float wildcard_log_weight, int B, int T, int V, int U,
                                        const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                                        int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_optional_wildcard_label_posterior_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes /*host*/);
int ctc_amd_optional_wildcard_label_posterior(int kind, int wrt,
                                              const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                              const int32_t *labels, int label_stride,
                                              const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                              float wildcard_log_weight, int B, int T, int V, int U,
                                              float *loss, float *label_posterior, float *blank_posterior, float *duration,
                                              float *expected_frame, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Optional wildcards above 1024 labels: the long-form loss, gradient and label posteriors (added under ABI v6: three new entry
 * points with their size queries, nothing existing changed).  CTC_AMD_OPTIONAL_WILDCARD with the definition above, word for word,
 * for label_length <= CTC_AMD_LONG_MAX_U, accepted by
 *   ctc_amd_long_optional_wildcard_loss_grad         counterpart: ctc_amd_long_wildcard_loss_grad
 *   ctc_amd_long_optional_wildcard_loss_grad_ckpt    counterpart: ctc_amd_long_wildcard_loss_grad_ckpt
 *   ctc_amd_long_optional_wildcard_label_posterior   counterpart: ctc_amd_long_label_posterior
 * Each is its counterpart in arguments, formats, strides, outputs, limits, validation order and messages, launches, capture and
 * determinism: the same bits on every run, for every frames_per_tile and batch composition, from both workspaces.  Two adjacent
 * optional wildcards make the utterance infeasible wherever the pair falls, a label-block boundary (positions 1023 / 1024)
 * included: loss +inf, zero gradient, zero posteriors, expected_frame -1.  A transcript without an optional wildcard returns the
 * counterpart's bits for every output; at one label block the loss, gradient, label_posterior, duration and expected_frame are
 * the bits of the short-form optional entry points.
 * Workspace.  A skip reaches two positions back, across a label-block boundary, so two more column buffers lie behind the
 * counterpart's workspace: with K = ceil(U / 1024) label blocks, 16 * B * (K - 1) * T bytes (the state of position k * 1024 - 2
 * before every frame) and, with a gradient or for the posteriors, 8 * B * (K - 1) * T more (what entering position
 * (k + 1) * 1024 + 1 with a frame is worth), each rounded up to 256.  The three size queries return the counterparts' sizes plus
 * those terms (K = 1: the same size).  The workspace may hold anything on entry.
 * Short utterances.  An utterance of L positions needs at least L / 2 frames, not L: the tiles that run are chosen by that bound
 * (position i is unreachable before frame i / 2), and what is infeasible beyond it falls out of the lattice.
 * Not included: the long-form alignment, the N-best calls, frame windows together with optional wildcards, and star temporal
 * classification's exclusion of the following label.
 */
int ctc_amd_long_optional_wildcard_loss_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, int want_grad,
                                                        size_t *out_bytes /*host*/);
int ctc_amd_long_optional_wildcard_loss_grad(int kind, int wrt,
                                             const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                             const int32_t *labels, int label_stride,
                                             const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                             float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                             const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                                             int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_long_optional_wildcard_loss_ckpt_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, int want_grad,
                                                             size_t *out_bytes /*host*/);
int ctc_amd_long_optional_wildcard_loss_grad_ckpt(int kind, int wrt,
                                                  const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                                  const int32_t *labels, int label_stride,
                                                  const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                                  float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                                  const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                                                  int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream);
int ctc_amd_long_optional_wildcard_label_posterior_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile,
                                                                   size_t *out_bytes /*host*/);
int ctc_amd_long_optional_wildcard_label_posterior(int kind, int wrt,
                                                   const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                                   const int32_t *labels, int label_stride,
                                                   const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                                   float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                                   float *loss, float *label_posterior /* may be NULL */, float *blank_posterior,
                                                   float *duration, float *expected_frame, float *peak_posterior, int32_t *peak_frame,
                                                   void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CTC_AMD_H */
