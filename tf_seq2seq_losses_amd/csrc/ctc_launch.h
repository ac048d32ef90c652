// Host launchers that cross a translation unit: every unit that defines or calls one includes this header, so a changed
// signature is a compile error in both places.  Host declarations only.
#pragma once
#include "ctc_common.h"

namespace ctc {

// ctc_kernels.hip: the three-kernel pipeline and the small kernels around it
hipError_t run_emit_scan(const Problem &p, const Layout &L, char *ws, float *loss, int ndir, hipStream_t st);
hipError_t run_grad(const Problem &p, const Layout &L, char *ws, const float *d_loss, float *grad, hipStream_t st);
hipError_t run_order(const Problem &p, const Layout &L, char *ws, hipStream_t st);  // longest utterances first, into L.off_perm
hipError_t run_sum_loss_fixed(const float *loss, int B, long long *acc, long long *zero_next, hipStream_t st);
hipError_t run_reduce_loss(const float *loss, int B, float *out, hipStream_t st);
hipError_t run_log_posterior(const Problem &p, const Layout &L, char *ws, float *out, hipStream_t st);
hipError_t run_convert(const Problem &p, const Layout &L, char *ws, float *alpha_out, float *beta_out, hipStream_t st);
hipError_t run_probe_copy(void *dst, const void *src, size_t bytes, hipStream_t st);
hipError_t run_probe_spin(int threads, int lds_bytes, float us, hipStream_t st);
hipError_t run_check_labels(const int32_t *labels, int label_stride, const int32_t *label_length, int blank, int B, int V, int U,
                            int *bad, hipStream_t st);

// ctc_fused5.hip / ctc_fused6.hip: one unit, and one entry point, per (lattice kind, label positions per lane NL)
typedef hipError_t FusedEntry(const Problem &p, const Layout &L, char *ws, float *loss, const float *d_loss, float *grad, hipStream_t st);
FusedEntry run_fused5_classic_nl1, run_fused5_classic_nl2, run_fused5_classic_nl4, run_fused5_classic_nl8;
FusedEntry run_fused5_simplified_nl1, run_fused5_simplified_nl2, run_fused5_simplified_nl4, run_fused5_simplified_nl8;
FusedEntry run_fused6_classic_nl1, run_fused6_classic_nl2, run_fused6_classic_nl4, run_fused6_classic_nl8;
FusedEntry run_fused6_simplified_nl1, run_fused6_simplified_nl2, run_fused6_simplified_nl4, run_fused6_simplified_nl8;

// ctc_hessian.hip
extern int g_force_hessian_slab;  // ctc_capi.hip (ctc_amd_debug_override "hessian")
size_t hessian_extra_bytes(int kind, int B, int T, int V, int U);
hipError_t run_hessian(const Problem &p, const Layout &L, char *ws, const float *g_lp, float *hess, hipStream_t st);

// ctc_hvp.hip, ctc_hvp_fused.hip (one unit per lattice kind)
size_t hvp_extra_bytes(int kind, int B, int T, int V, int U);
size_t hvp_fused_flags_offset(int kind, int B, int T, int U);
hipError_t run_hvp(const Problem &p, const Layout &L, char *ws, const float *vec, float *out, hipStream_t st);
hipError_t run_hvp_fused_classic(const Problem &p, const Layout &L, char *ws, const float *vec, float *loss, float *out, int mode, hipStream_t st);
hipError_t run_hvp_fused_simplified(const Problem &p, const Layout &L, char *ws, const float *vec, float *loss, float *out, int mode, hipStream_t st);

// ctc_align.hip: best-path (Viterbi) alignment; the workspace holds the back-pointers alone ([B][T][64] words of 1 .. 8 bytes)
size_t align_workspace_bytes(int B, int T, int U);
hipError_t run_align(const Problem &p, char *ws, float *score, int *tokens, int *label_index, hipStream_t st);

// ctc_decode.hip: greedy decoding; the workspace holds the float32 log-probability of every frame's token ([B][T])
size_t decode_workspace_bytes(int B, int T);
hipError_t run_decode(const Problem &p, char *ws, float *score, int *tokens, int *decoded, int *decoded_length, int *frames,
                      float *label_score, hipStream_t st);

// ctc_nbest.hip: exact loss of N hypotheses per utterance; one workgroup per utterance and group of NBEST_G hypotheses
// (= CTC_AMD_NBEST_GROUP, include/ctc_amd.h).  Everything lives in registers and LDS: no workspace (the size is 0 bytes)
constexpr int NBEST_G = 8;
size_t nbest_workspace_bytes(int kind, int B, int T, int V, int U, int N);
hipError_t run_nbest(const Problem &p, int N, float *loss, hipStream_t st);
// ... and the gradient of sum_n weight[b, n] * loss[b, n]: alpha sweep that keeps its rows, beta sweep, row stage.  The workspace
// holds the float64 rows of every hypothesis and frame, the row statistics and log2 P
size_t nbest_grad_workspace_bytes(int kind, int B, int T, int V, int U, int N);
hipError_t run_nbest_grad(const Problem &p, int N, const float *weight, float *loss, void *grad, char *ws, hipStream_t st);

// ctc_edit.hip: edit distance of every hypothesis (b, n) to its utterance's reference; one wavefront per pair, one launch, no workspace
hipError_t run_edit_distance(const int *hyp, int hyp_stride, const int *hyp_length, const int *ref, int ref_stride, const int *ref_length,
                             int B, int N, int R, int *distance, hipStream_t st);

// ctc_edit_long.hip: (distance, substitutions, insertions, deletions) of every pair for references of up to 65536 tokens; the table
// is tiled over blocks of 1024 reference tokens x plan.RT hypothesis tokens, one launch per anti-diagonal of tiles; the workspace
// holds the tiles' boundary rows and columns (ctc_edit_long_plan.h)
struct EditCountsPlan;
hipError_t run_edit_counts(const int *hyp, int hyp_stride, const int *hyp_length, const int *ref, int ref_stride, const int *ref_length,
                           int N, const EditCountsPlan &plan, int *counts, char *ws, hipStream_t st);

#ifdef CTC_WIDE_EXPERIMENT
// experiments/wide/ctc_wide.hip: parked outside the product tree, built by experiments/wide/build_wide_variant.sh only
extern int g_wide_diag;  // timing diagnostics (results are then meaningless)
bool wide_eligible(const Problem &p, const Layout &L);
hipError_t run_wide(const Problem &p, const Layout &L, char *ws, float *loss, const float *d_loss, float *grad, hipStream_t st);
#endif

}  // namespace ctc
